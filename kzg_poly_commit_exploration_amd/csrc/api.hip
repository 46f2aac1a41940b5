// api.hip -- the C-ABI of libkzg_mi355x.so (declared in include/kzg_mi355x.h): context, SRS
// residency, job slots and the three streams, the host-side orchestration of one commitment / opening, and the serial
// tail (a few dozen point additions + one inversion) that finishes each MSM on the host.
//
// One commitment, over the context's three streams (front: up to the sort; accumulation; tail: from the finalisation on):
//   digits+histogram -> scan -> scatter -> bucket accumulation -> bucket finalisation
//   -> row / column tree sums of the bucket matrix, split once more (small jobs: one launch behind the sort)
//   -> D2H of <= 128 XYZZ partials -> host: four short weighted sums, normalise, blst_p1 out.
// Nothing here falls back to the CPU for the MSM or the division: without a device the context
// cannot be created.
#include <hip/hip_runtime.h>
#include <sys/random.h>

#include <algorithm>
#include <atomic>
#include <cerrno>
#include <chrono>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <functional>
#include <mutex>
#include <new>
#include <string>
#include <thread>
#include <vector>

#include "../../include/kzg_mi355x.h"
#include "engine.h"
#include "host_field.hpp"
#include "host_fr.hpp"
#include "fr30_host.hpp"
#include "host_pairing.hpp"
#include "host_sha256.hpp"
#include "wire30.hip.h"

using namespace kzg;
namespace hf = kzg_host;

namespace {

// The reference refuses polynomials of more than u32::MAX coefficients (src/polynomial.rs:56-61); the kernels index
// with 32 bits, so the C-ABI refuses them too instead of truncating the count.
constexpr size_t kMaxCoefficients = 0xFFFFFFFFull;

// Job slots per context: a slot is a job's workspaces, events, flag words and bookkeeping.  The streams belong to the
// context, one per phase (kzg_ctx below), so the number of slots does not decide the number of hardware queues in use.  The
// light kernels of a job -- sort in front of its accumulation, finalisation and reduction trees behind it -- only get
// the chip in the tail of ANOTHER job's accumulation and crawl while one is running (round-3 timeline: a 54 us sort
// kernel takes 260, the trees 1 ms).  With three jobs in flight the next job's sort regularly finished 100-240 us after
// the accumulation it should have hidden under; five give it one more accumulation's worth of time: 366 -> 389
// commitments/s on the same box (4: 383-390, 6: 381-385, 7: 368-385).
#ifndef KZG_NUM_SLOTS
#define KZG_NUM_SLOTS 5
#endif
constexpr int kNumSlots = KZG_NUM_SLOTS;
// Reduction plan (msm_reduce.hip): bucket index b = hi * C + lo; Row (R entries) and Col (C entries)
// are each split once more into a "row" part and a "column" part that the host receives.
struct ReducePlan {
    uint32_t lo_bits = 0, hi_bits = 0;  // C = 2^lo_bits, R = 2^hi_bits
    uint32_t row_lo = 0, row_hi = 0;    // split of the Row vector index (hi_bits = row_lo + row_hi)
    uint32_t col_lo = 0, col_hi = 0;    // split of the Col vector index (lo_bits = col_lo + col_hi)
    // record offsets inside the final buffer
    uint32_t off_r2row = 0, off_c2row = 0, off_r2col = 0, off_c2col = 0, total = 0;
};

// what a slot holds decides which wait entry point may collect it (a batched job's final buffer is laid out
// [section][polynomial][record]; reading it as a single job would return a wrong point with KZG_OK)
// SLOT_RESERVED: owned by a synchronous host-pointer call between its steps (upload -> submit -> wait), during which the
// context mutex is NOT held: N caller threads occupy N slots and their jobs pipeline like explicit submits do.
enum SlotKind { SLOT_IDLE = 0, SLOT_COMMIT = 1, SLOT_OPEN = 2, SLOT_TRIVIAL = 3, SLOT_COMMIT_BATCH = 4, SLOT_OPEN_BATCH = 5, SLOT_RESERVED = 6,
                SLOT_OPEN_POINTS = 7 /* a multiproof: trivial or not, collected by kzg_wait */,
                SLOT_OPEN_COMBINED = 8 /* a combined opening: trivial or not, collected by kzg_wait_combined */,
                SLOT_OPEN_SETS = 9 /* an opening at several point sets: trivial or not, collected by kzg_wait_sets */ };

// Sets ctx->last_error to "<what>: <HIP's text>" and returns KZG_ERR_HIP, as HIP_TRY does (defined below kzg_ctx).
int hip_fail(kzg_ctx* ctx, const char* what, hipError_t e);

// ---- the owners of the context's device and pinned memory -----------------------------------------
// Both free in their destructor, cannot be copied, and have ONE way to get memory: reserve(), which does nothing when the
// request fits and otherwise waits for `drain` (the stream whose queued work may still read the old block; none for callers
// that have waited already), frees, and allocates exactly `bytes`.  Growth DROPS the contents.  After a failed allocation the
// owner is empty (null, capacity 0).  dev<T>() / host<T>() are the typed views the launchers take.
struct DevBuf {
    void* p = nullptr;
    size_t cap = 0;  // bytes of the last reserve() (0 where a setup path filled p itself)
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    ~DevBuf() { reset(); }
    void reset() {
        if (p) hipFree(p);
        p = nullptr;
        cap = 0;
    }
    template <class T = uint32_t> T* dev() const { return (T*)p; }
    int reserve(kzg_ctx* ctx, size_t bytes, hipStream_t drain = nullptr) { return bytes <= cap ? KZG_OK : grow(ctx, bytes, drain); }
    int grow(kzg_ctx* ctx, size_t bytes, hipStream_t drain) {
        if (drain)
            if (hipError_t e = hipStreamSynchronize(drain)) return hip_fail(ctx, "hipStreamSynchronize", e);
        reset();
        if (hipError_t e = hipMalloc(&p, bytes)) {
            p = nullptr;
            return hip_fail(ctx, "hipMalloc", e);
        }
        cap = bytes;
        return KZG_OK;
    }
};
// A pinned host block with its device side.  Mapped: the device side is the block's own device address (the kernels write
// the host's memory directly: flag words, values, the MSM's last partial sums).  Staged: the device side is a device buffer
// of the same size that the caller fills with a copy on its stream.
struct PinnedBuf {
    enum Kind { Mapped, Staged };
    const Kind kind;
    void *h = nullptr, *d = nullptr;
    size_t cap = 0;
    explicit PinnedBuf(Kind k) : kind(k) {}
    PinnedBuf(const PinnedBuf&) = delete;
    PinnedBuf& operator=(const PinnedBuf&) = delete;
    ~PinnedBuf() { reset(); }
    void reset() {
        if (h) hipHostFree(h);
        if (d && kind == Staged) hipFree(d);
        h = d = nullptr;
        cap = 0;
    }
    template <class T = uint32_t> T* host() const { return (T*)h; }
    template <class T = uint32_t> T* dev() const { return (T*)d; }
    int reserve(kzg_ctx* ctx, size_t bytes, hipStream_t drain = nullptr) { return bytes <= cap ? KZG_OK : grow(ctx, bytes, drain); }
    int grow(kzg_ctx* ctx, size_t bytes, hipStream_t drain) {
        if (drain)
            if (hipError_t e = hipStreamSynchronize(drain)) return hip_fail(ctx, "hipStreamSynchronize", e);
        reset();
        hipError_t e = hipHostMalloc(&h, bytes, kind == Mapped ? hipHostMallocMapped : hipHostMallocDefault);
        if (e == hipSuccess) e = kind == Mapped ? hipHostGetDevicePointer(&d, h, 0) : hipMalloc(&d, bytes);
        if (e != hipSuccess) {
            d = nullptr;
            reset();
            return hip_fail(ctx, kind == Mapped ? "hipHostMalloc (mapped)" : "hipHostMalloc + hipMalloc (staging)", e);
        }
        cap = bytes;
        return KZG_OK;
    }
};
// The workspaces of one feature, grown on demand under that feature's mutex (its callers have waited for the stream before
// they ask again: no drain).  A request of 0 bytes still hands out a valid pointer (256 bytes, recorded as 0).
template <int N>
struct Workspace {
    DevBuf buf[N];
    int get(kzg_ctx* ctx, int i, size_t bytes, void** out) {
        DevBuf& b = buf[i];
        int rc = KZG_OK;
        if (!bytes && !b.p) {
            rc = b.reserve(ctx, 256);
            b.cap = 0;
        } else {
            rc = b.reserve(ctx, bytes);
        }
        *out = b.p;
        return rc;
    }
};

// A slot's events and its view of the context's streams.  They are the base of Slot, so the events are destroyed AFTER the
// slot's buffers (members go first): kzg_ctx_destroy waits for the streams, `delete` frees the buffers, then the events go.
struct SlotQueue {
    hipStream_t stream = nullptr;  // the context's front stream (every slot holds the same one; the context destroys it)
    hipStream_t end = nullptr;     // where the job in flight ended: the front stream, or the tail stream after a hand-over
                                   // (set by enqueue_msm); `done` and the job's last timing event are recorded there
    hipEvent_t ev[8] = {};
    hipEvent_t done = nullptr;
    hipEvent_t sorted_ev = nullptr, accum_ev = nullptr;  // hand-offs to / from the shared accumulation stream
    hipEvent_t cmb_ev[2] = {};                           // timed combined openings: around the (last) combination pass
    hipEvent_t cells_ev = nullptr;                       // kzg_cells_and_proofs: P is in cpoly
    hipEvent_t upload_ev = nullptr;                      // host-pointer calls: the coefficients are in the slot (upload stream)
    SlotQueue() = default;
    SlotQueue(const SlotQueue&) = delete;
    SlotQueue& operator=(const SlotQueue&) = delete;
    ~SlotQueue() {
        for (hipEvent_t e : {ev[0], ev[1], ev[2], ev[3], ev[4], ev[5], ev[6], ev[7], cmb_ev[0], cmb_ev[1], cells_ev, upload_ev, done, sorted_ev, accum_ev})
            if (e) hipEventDestroy(e);
    }
};

struct Slot : SlotQueue {
    // MSM workspace (sized at SRS load)
    DevBuf cnt, offs, block_sums, pairs, sorted, buckets;
    DevBuf recoded;         // the folded scalars of the job, 32 bytes each: written by the sort's first pass, read by its second
    DevBuf part_a, part_b;  // head / tail partials of the accumulation segments
    DevBuf pair_scratch;    // prefix products of the affine front end (msm_accum.hip)
    DevBuf heavy_ws;        // long-bucket registry + tree buffers of msm_finalize.hip
    DevBuf arena;           // Row[] then Col[] vectors of the bucket matrix
    // The <= 128 partial sums the host finishes are written by the last reduction kernel STRAIGHT into pinned host
    // memory: a copy back is a blit kernel on this runtime, and behind an accumulation kernel that fills the chip it took
    // 1.3 ms instead of 5 us -- the host collected the job that much later, submitted the next one that much later, and
    // its sort finished after the accumulation it should have hidden under (100-240 us of idle chip per commitment;
    // round-3 timeline).
    PinnedBuf fin{PinnedBuf::Mapped};
    // polynomial workspace (grown on demand, all four together: ensure_poly)
    DevBuf stage;  // coefficients copied from the host
    DevBuf q;      // quotient
    DevBuf chunk, block;
    // The job's flag words live in pinned host memory that the kernels write directly (plain stores only -- every writer
    // of a flag stores the same 1): no memset and no copy-back on the stream.  A 256-byte copy back is a blit kernel here,
    // and queued behind a chip-filling accumulation it sat for ~1 ms between the job's last kernel and the moment the host
    // could collect it.
    PinnedBuf small{PinnedBuf::Mapped};   // [0..1] flags, [8..15] P(z), [16..23] c0, [24] tail flag, [26] references
    PinnedBuf bsmall{PinnedBuf::Mapped};  // batched openings: 32 words per polynomial, same layout as small[0..31]
    std::vector<uint32_t> open_ys;  // y of every polynomial of a batched opening (8 words each)
    // multiproofs (kzg_open_points): the per-root multipliers are copied on the front stream (a slot holds one job at a
    // time, so nothing in flight reads them while they are rewritten); the k values P(z_i) land in mapped memory like the
    // flag words; pblock: k x nblocks aggregates
    PinnedBuf roots{PinnedBuf::Staged};
    PinnedBuf pvals{PinnedBuf::Mapped};
    DevBuf pblock;
    std::vector<uint32_t> pts_ys;  // the claims (8 words each)
    size_t pts_nq = 0;             // terms of the job's MSM (0: the proof is infinity once the claims hold)
    // combined openings (kzg_open_combined): the call's multipliers (powers of z, gamma^i) in ctab,
    // the t values P_i(z) in cvals; F is built in stage.  cpart: the (polynomial, tile) records of one pass; cin: the
    // polynomials of one pass of the host-pointer call.
    PinnedBuf ctab{PinnedBuf::Staged};
    PinnedBuf cvals{PinnedBuf::Mapped};
    DevBuf cpart, cin;
    size_t cmb_t = 0;  // polynomials of the job in flight
    float combine_ms = 0;
    // openings at several point sets (kzg_open_sets): the pass tables (66 powers per distinct point,
    // then one multiplier per (point, polynomial opened there)) in stab and the selection lists in ssel; the values land in
    // svals in pass order and sets_vmap says where each entry of out_ys sits; sg: the G_p, |T| x n values.  The passes share
    // cpart / cin, the scans the multiproof's root and aggregate buffers.
    PinnedBuf stab{PinnedBuf::Staged}, ssel{PinnedBuf::Staged};
    PinnedBuf svals{PinnedBuf::Mapped};
    DevBuf sg;
    std::vector<uint32_t> sets_vmap;
    // the last round of a circuit's proof (kzg_circuit_open): the column records of k_lin_combine, one
    // table of kLinMaxColumns per distinct point
    PinnedBuf ltab{PinnedBuf::Staged};
    // ... with blinders (kzg_circuit_open_blinded): per distinct point the column records of k_blind_tail and
    // the powers of the point, then the blinders the records point at
    PinnedBuf btab{PinnedBuf::Staged};
    // openings from evaluations over the Lagrange basis (kzg_open_lagrange): the tile records of the
    // quotient kernels; the quotient's values go to q
    DevBuf lag_part;
    // grand products (kzg_grand_product and the permutation forms): the columns of a host-pointer call
    // (numerators then denominators, packed to stride n), its z, the tile records, and the two results the carry kernel writes
    // for the host: [0] the least index with a zero denominator, [8..15] z_n
    DevBuf gp_in, gp_z, gp_part;
    PinnedBuf gp_flags{PinnedBuf::Mapped};
    // cells of a domain (kzg_cells_and_proofs): P for the whole call in cpoly (read by the sub-batches of every slot the call
    // holds, after cells_ev), the chunk aggregates of the cell quotients in cagg
    DevBuf cpoly, cagg;
    // multilinear openings (kzg_ml_fold, kzg_ml_open): the values and the pyramid of a host-pointer call
    DevBuf ml_in, ml_pyr;
    // state of the job in flight
    SlotKind kind = SLOT_IDLE;
    size_t job_n = 0;
    uint32_t job_batch = 1;
    uint32_t open_y[8] = {};
    bool timing = false;
    bool has_quotient = false;
    bool tail_checked = false;
    kzg_kernel_times times = {};
};

}  // namespace

struct kzg_ctx {
    // a multi-device context (kzg_ctx_create_multi) only carries this pointer: its calls are sharded over the
    // single-device contexts inside (multi.hip)
    kzg::MultiState* multi = nullptr;
    int device = 0;
    std::mutex mu;
    std::condition_variable slot_cv;  // a slot became idle / a synchronous call finished
    int sync_owned = 0;               // slots currently owned by synchronous host-pointer calls (reserve_slot)
    bool raw_partials = false;        // kid of a range-split multi-device context: results stay un-normalised (ctx_set_raw_partials)
    // KZG_HOST_TRACE=1: where a synchronous host-pointer call spends its wall time (printed when the context is destroyed)
    bool host_trace = false;
    std::atomic<uint64_t> trace_ns[5] = {};  // reserve (waiting for a slot), upload, submit, device wait, collect (host tail)
    std::atomic<uint64_t> trace_calls{0};
    std::string last_error;
    // SRS
    size_t n = 0;  // points
    MsmConfig cfg = {};
    DevBuf table;   // W * n affine points
    bool nttb_ready = false;  // the batched pass kernel's LDS limit is raised (ensure_ntt_batch)
    DevBuf ntt_tw;  // NTT twiddles, built on first use: forward lo, forward hi, inverse lo, inverse hi (ntt_kernels.hip)
    // The Lagrange basis of one domain: L_i = [l_i(s)] G1 for the lag_n = 2^k points of the domain, with
    // its own window-table levels in the SRS table's format (level stride lag_n, the same MsmConfig, lag_n <= n so the slots'
    // workspaces fit).  Built under fk20_mu (the DFT reads the split twiddles) by kzg_lagrange_prepare or the first host-pointer
    // call that needs it; dropped with the SRS (srs_release).
    DevBuf lag_table;
    size_t lag_n = 0;
    uint64_t srs_gen = 0;  // counts the SRS replacements (srs_release): a basis built across one is not adopted
    ReducePlan plan;
    size_t arena_records = 0, final_records = 0;  // per polynomial of a batch
    uint32_t max_batch = 1;                        // polynomials per submit the workspaces are sized for
    Slot slots[kNumSlots];
    // Three streams, one per phase of a job, at any number of slots -- they fit the four hardware queues a process gets by
    // default however the runtime assigns them, so neither results nor rate depend on the queue count:
    //   front_stream (lowest priority): everything a job enqueues before its accumulation (quotient or combination passes,
    //     the degree check, the sort), the one-launch small jobs in full, and every other feature's copies and kernels.
    //     Every slot's `stream` member is this stream.
    //   heavy_stream (highest priority): all bucket-accumulation kernels, in submission order: each fills the chip on its
    //     own, so letting two of them overlap only makes both slower (and their timings meaningless), while the light
    //     kernels of the other jobs run beside it.  Waits for the job's sorted_ev, records its accum_ev.
    //   tail_stream (lowest priority): waits for accum_ev, then the finalisation and the tree sums; the job's `done`.
    // THE INVARIANT: no operation that waits for an accumulation or for a tail is ever enqueued on the front stream (a job
    // that found every other slot idle runs on it in full, hand-overs saved: nothing was there to wait).  So the next
    // job's sort never stands behind a pending tail, whichever streams share a hardware queue.  A job is ordered behind the
    // previous job of its slot by the host: a slot is reused only after it was collected (its `done` event waited for).
    hipStream_t front_stream = nullptr, heavy_stream = nullptr, tail_stream = nullptr;
    // The coefficients of the host-pointer commitments and openings (kzg_commit, kzg_open, kzg_open_points, the batches) go
    // up on a stream of their own (default priority: a queue from another pool than the three above) and the front stream
    // waits for the slot's upload_ev.  A copy from pageable memory returns when it is done, and on the front stream it is
    // done only after every sort and quotient queued before it: with four caller threads the uploads stood behind each
    // other's kernels (380 against the parent's 395 proofs/s).  Nothing but copies is ever enqueued on it.
    hipStream_t upload_stream = nullptr;
    // LDS reserved per accumulation workgroup (KZG_ACCUM_LDS_KB overrides): 41 KB would cap the kernel at three workgroups
    // per CU; its register count (176 reserved, msm_accum.hip) caps it at two, which is what its grid is launched for.
    // Two workgroups leave 78 KB of LDS and 160 VGPRs per SIMD lane to the light kernels of the other slots (32 KB instead
    // of 41 measured the same).
    uint32_t accum_lds_bytes = 41u * 1024u;
    uint32_t small_lds_bytes = 48u * 1024u;  // k_small_msm's LDS reservation (raised to small_msm_lds_bytes() at creation)
    bool small_msm_off = false;              // KZG_SMALL_MSM=0: small jobs take the general multi-launch path (A/B, tests)
    // the four transform buffers of one pass of the quotient calls together stay below this (KZG_PQ_WS_KB lowers it, so that
    // tests turn the pass loops of pq_extend and coset_extend_impl at small shapes)
    size_t pq_ws_budget = (size_t)1 << 30;
    bool slots_ready = false;
    bool timing = false;
    // FK20 (kzg_cells_and_proofs_fk20), all under fk20_mu (taken before mu): the GLV-split twiddles
    // of w_(2^glv_log), built on first use and grown; the SRS side of one shape (L = 2^fk20_log_L, l = 2^fk20_log_l): the
    // transforms DFT_L(S_r) in fk20_B and, when they fit the budget, their comb tables in fk20_tab (both dropped with
    // the SRS); workspaces grown on demand
    std::mutex fk20_mu;
    DevBuf glv;
    uint32_t glv_log = 0;
    DevBuf fk20_B, fk20_tab;
    uint32_t fk20_log_L = 0, fk20_log_l = 0;
    Workspace<11> fk20_ws;
    // recovery (kzg_recover_cells_and_proofs), under recover_mu (taken before mu): the g-power tables
    // g^i, g^-i (g = 7) in the NTT twiddles' lo / hi shape, built on first use; workspaces grown on demand
    std::mutex recover_mu;
    DevBuf rec_g;
    Workspace<11> rec_ws;
    // batch verification of cells (kzg_verify_cells_batch): workspaces grown on demand, under fk20_mu
    // (the call reads the split twiddles glv, which an FK20 call may grow)
    Workspace<17> vc_ws;
    // the producing side on blob bytes (kzg_blobs_to_cells_and_proofs_bytes): workspaces grown on demand,
    // under fk20_mu (the calls run FK20 from them)
    Workspace<8> blob_ws;
    // the quotient of a permutation argument (kzg_coset_extend .. kzg_permutation_quotient), under
    // quotient_mu (taken before mu): workspaces grown on demand; the calls read the g-power tables rec_g, which are built once
    // and never replaced
    // lookups (kzg_lookup_multiplicities), under lookup_mu (taken before mu): the hash table's slots and
    // flag words, the counts, and the columns and outputs of a host-pointer call; grown on demand.  The sums and the batch
    // inverse use the slot's grand-product buffers instead (a slot holds one job at a time).
    std::mutex lookup_mu;
    Workspace<6> lu_ws;
    std::mutex quotient_mu;
    Workspace<13> pq_ws;
    DevBuf prove_buf[5];  // kzg_circuit_prove's cross-round buffers (values, coefficients, blinded copies, T, blinders): grown, kept
    uint32_t pq_zinv_key = ~0u;  // (log n << 8) | log rot of the inverses of Z_H held in pq_ws, ~0: none
    // the circuits alive on this context (kzg_circuit_create), under quotient_mu: kzg_ctx_destroy frees
    // what the caller left
    std::vector<kzg_circuit*> circuits;
};

// A circuit's key: the 2 t + 2 columns q_lin[0..t), q_mul, q_const, sigma[0..t) in that order, in three
// forms, every one as blst_fr images and every buffer the circuit's own, written by kzg_circuit_create and read-only afterwards.
// A lookup circuit (kzg_circuit_create_lookup, section 4.26) keeps c_tab + 1 more columns behind them, tab[0..c_tab) and q_K,
// which every call of section 4.22 .. 4.25 ignores.
// `owner` is the single-device context it lives on (devices[0]'s for a multi-device context).
struct kzg_circuit {
    kzg_ctx* owner = nullptr;
    uint32_t lg_n = 0, lg_ext = 0;
    size_t n = 0, t = 0;
    size_t c_tab = 0;  // table columns of a lookup circuit, 0: none
    // a custom circuit (kzg_circuit_create_custom, section 4.27; never with a table): g_custom selector columns qx_s behind the
    // 2 t + 2, the exponents p[s][j] at s t + j and the largest row sum; calls of section 4.22 .. 4.25 ignore them too
    size_t g_custom = 0, d_max = 0;
    uint8_t exps[kCgMaxTerms * kPqMaxColumns] = {};
    // a next-row circuit (kzg_circuit_create_custom_next, section 4.28): the second matrix p'[s][j] at s t + j, and the rho >= 1
    // wires with a next-row exponent, ascending (rho = 0: a custom circuit of section 4.27, or none); d_max counts both matrices
    uint8_t exps_next[kCgMaxTerms * kPqMaxColumns] = {};
    size_t rho = 0;
    uint8_t next_wires[kPqMaxColumns] = {};
    uint64_t shifts[4 * kPqMaxColumns] = {};
    DevBuf values;  // cols() x n
    DevBuf coeffs;  // cols() x n
    DevBuf coset;   // cols() x N
    DevBuf l0;      // the N values of L_0 on the coset
    DevBuf zinv;    // the rot stored multipliers 1 / Z_H(x_i): the circuit's own copy, independent of pq_zinv_key
    size_t N() const { return n << lg_ext; }
    size_t cols() const { return 2 * t + 2 + (c_tab ? c_tab + 1 : 0) + g_custom; }
};

namespace {

#define HIP_TRY(ctx, expr)                                                                          \
    do {                                                                                            \
        hipError_t _e = (expr);                                                                     \
        if (_e != hipSuccess) {                                                                     \
            (ctx)->last_error = std::string(#expr) + ": " + hipGetErrorString(_e);                  \
            return KZG_ERR_HIP;                                                                     \
        }                                                                                           \
    } while (0)

int hip_fail(kzg_ctx* ctx, const char* what, hipError_t e) {
    ctx->last_error = std::string(what) + ": " + hipGetErrorString(e);
    return KZG_ERR_HIP;
}

// scope guard for the setup paths (several HIP_TRY early returns; their buffers are DevBufs)
struct TmpStream {
    hipStream_t s = nullptr;
    ~TmpStream() { if (s) hipStreamDestroy(s); }
};

// Waits for the (front) stream without ctx->mu, so that the context's other calls go on meanwhile (the caller's slot keeps an SRS
// replacement out, its feature's mutex the other calls of its kind).  `what` starts the text an error leaves.
int sync_unlocked(kzg_ctx* ctx, std::unique_lock<std::mutex>& lk, hipStream_t st, const char* what) {
    lk.unlock();
    const hipError_t e = hipStreamSynchronize(st);
    lk.lock();
    return e == hipSuccess ? KZG_OK : hip_fail(ctx, what, e);
}
// A copy on the stream without ctx->mu (pageable host memory: the call may block).
constexpr const char* kCopyCoeffs = "hipMemcpyAsync (coefficients)";
int copy_unlocked(kzg_ctx* ctx, std::unique_lock<std::mutex>& lk, hipStream_t st, void* dst, const void* src, size_t bytes,
                  hipMemcpyKind kind, const char* what) {
    if (!bytes) return KZG_OK;
    lk.unlock();
    const hipError_t e = hipMemcpyAsync(dst, src, bytes, kind, st);
    lk.lock();
    return e == hipSuccess ? KZG_OK : hip_fail(ctx, what, e);
}

void free_slot_msm(Slot& s) {
    for (DevBuf* b : {&s.cnt, &s.offs, &s.block_sums, &s.pairs, &s.recoded, &s.sorted, &s.buckets, &s.part_a, &s.part_b, &s.pair_scratch,
                      &s.heavy_ws, &s.arena})
        b->reset();
    s.fin.reset();
}

// one of the context's streams: the highest or the lowest priority (KZG_STREAM_PRIORITIES=0: the default one for all)
int create_stream(kzg_ctx* ctx, hipStream_t* out, bool high) {
    int least = 0, greatest = 0;
    HIP_TRY(ctx, hipDeviceGetStreamPriorityRange(&least, &greatest));
    const char* v = std::getenv("KZG_STREAM_PRIORITIES");
    const bool prio = !(v && v[0] == '0');
    HIP_TRY(ctx, hipStreamCreateWithPriority(out, hipStreamNonBlocking, prio ? (high ? greatest : least) : 0));
    return KZG_OK;
}

// the front stream, events and the small flag buffers of a slot (what kzg_quotient / kzg_evaluate need without an SRS)
int ensure_slot_basics(kzg_ctx* ctx, Slot& s) {
    if (s.stream) return KZG_OK;
    // the front and tail streams run the light kernels (sort, quotient; finalise, reduction): lowest priority, so that
    // when an accumulation ends the NEXT accumulation (high-priority stream) takes the chip first and the
    // ~180-VGPR reduction kernels fill in behind it instead of holding half of every SIMD's registers
    if (!ctx->front_stream) {
        int rc = create_stream(ctx, &ctx->front_stream, false);
        if (rc) return rc;
    }
    if (!ctx->upload_stream) HIP_TRY(ctx, hipStreamCreateWithFlags(&ctx->upload_stream, hipStreamNonBlocking));
    for (auto& e : s.ev)
        if (!e) HIP_TRY(ctx, hipEventCreate(&e));
    if (!s.upload_ev) HIP_TRY(ctx, hipEventCreateWithFlags(&s.upload_ev, hipEventDisableTiming));
    s.stream = s.end = ctx->front_stream;
    if (!s.done) HIP_TRY(ctx, hipEventCreateWithFlags(&s.done, hipEventDisableTiming));
    return s.small.reserve(ctx, 64 * 4);
}

// The coefficients of a host-pointer job into the slot (dst: a part of s.stage that nothing in flight reads -- the slot's
// last job was collected): the copy on the upload stream without ctx->mu, then the front stream waits for it.
int upload_unlocked(kzg_ctx* ctx, std::unique_lock<std::mutex>& lk, Slot& s, void* dst, const void* src, size_t bytes) {
    if (!bytes) return KZG_OK;
    int rc = copy_unlocked(ctx, lk, ctx->upload_stream, dst, src, bytes, hipMemcpyHostToDevice, kCopyCoeffs);
    if (rc) return rc;
    HIP_TRY(ctx, hipEventRecord(s.upload_ev, ctx->upload_stream));
    HIP_TRY(ctx, hipStreamWaitEvent(s.stream, s.upload_ev, 0));
    return KZG_OK;
}

// the four polynomial buffers grow together, to at least 1024 coefficients
int ensure_poly(kzg_ctx* ctx, Slot& s, size_t n) {
    const size_t cap = n < 1024 ? 1024 : n;
    if (cap * 32 <= s.stage.cap) return KZG_OK;
    // nothing may still read the old buffers: the slot's last job has ended (its owner collected it; a failed submit may
    // have left a part of one in flight) and the upload and front streams, where every other user of these four runs, are empty
    if (s.done) HIP_TRY(ctx, hipEventSynchronize(s.done));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->upload_stream));
    HIP_TRY(ctx, hipStreamSynchronize(s.stream));
    for (DevBuf* b : {&s.stage, &s.q, &s.chunk, &s.block}) b->reset();
    int rc = s.stage.reserve(ctx, cap * 32);
    if (rc == KZG_OK) rc = s.q.reserve(ctx, cap * 32);
    if (rc == KZG_OK) rc = s.chunk.reserve(ctx, poly_chunk_words((uint32_t)cap) * 4);
    if (rc == KZG_OK) rc = s.block.reserve(ctx, poly_block_words((uint32_t)cap) * 4);
    if (rc) s.stage.reset();  // (its capacity stands for all four)
    return rc;
}

// reduction plan: depends only on the bucket count
void plan_reduce(kzg_ctx* ctx) {
    ReducePlan P;
    uint32_t bits = 0;  // log2(buckets)
    while ((1u << bits) < ctx->cfg.nb) bits++;
    P.lo_bits = bits / 2;
    P.hi_bits = bits - P.lo_bits;
    P.row_lo = P.hi_bits / 2;
    P.row_hi = P.hi_bits - P.row_lo;
    P.col_lo = P.lo_bits / 2;
    P.col_hi = P.lo_bits - P.col_lo;
    P.off_r2row = 0;
    P.off_c2row = P.off_r2row + (1u << P.row_hi);
    P.off_r2col = P.off_c2row + (1u << P.row_lo);
    P.off_c2col = P.off_r2col + (1u << P.col_hi);
    P.total = P.off_c2col + (1u << P.col_lo);
    ctx->plan = P;
    ctx->arena_records = ((size_t)1 << P.hi_bits) + ((size_t)1 << P.lo_bits);
    ctx->final_records = P.total;
}

int setup_slots_impl(kzg_ctx* ctx);
// (Re)allocates every slot's MSM workspace.  On any failure the context is left WITHOUT an SRS (n = 0, no
// workspaces, slots_ready false): the next commit returns KZG_ERR_NO_SRS instead of launching on freed buffers.
int setup_slots(kzg_ctx* ctx, bool keep_table_on_failure = false) {
    ctx->slots_ready = false;
    int rc = setup_slots_impl(ctx);
    if (rc != KZG_OK) {
        for (auto& s : ctx->slots) free_slot_msm(s);
        if (keep_table_on_failure) return rc;  // the caller retries with the previous sizes
        ctx->table.reset();
        ctx->lag_table.reset();
        ctx->lag_n = 0;
        ctx->n = 0;
        (void)hipGetLastError();
    }
    return rc;
}
int setup_slots_impl(kzg_ctx* ctx) {
    plan_reduce(ctx);
    if (const char* v = std::getenv("KZG_TEST_FAIL_SLOT_ALLOC")) {  // fault injection for tests/test_gpu_parity.py
        const int mode = std::atoi(v);  // 1: every setup fails; 2: only setups for more than one polynomial per batch
        if (mode == 1 || (mode == 2 && ctx->max_batch > 1)) {
            ctx->last_error = "injected allocation failure (KZG_TEST_FAIL_SLOT_ALLOC)";
            return KZG_ERR_HIP;
        }
    }
    if (!ctx->heavy_stream) {
        int rc = create_stream(ctx, &ctx->heavy_stream, true);
        if (rc) return rc;
    }
    if (!ctx->tail_stream) {
        int rc = create_stream(ctx, &ctx->tail_stream, false);
        if (rc) return rc;
    }
    const MsmConfig cfg = ctx->cfg;
    if (ctx->max_batch > sort_max_batch(cfg)) ctx->max_batch = sort_max_batch(cfg);
    const size_t B = ctx->max_batch;
    const size_t pairs = (size_t)cfg.max_digits * ctx->n * B;
    for (int i = 0; i < kNumSlots; i++) {
        Slot& s = ctx->slots[i];
        {
            int rcb = ensure_slot_basics(ctx, s);
            if (rcb) return rcb;
        }
        if (!s.sorted_ev) {
            HIP_TRY(ctx, hipEventCreateWithFlags(&s.sorted_ev, hipEventDisableTiming));
            HIP_TRY(ctx, hipEventCreateWithFlags(&s.accum_ev, hipEventDisableTiming));
        }
        free_slot_msm(s);
        int rc = s.cnt.reserve(ctx, (size_t)sort_count_entries((uint32_t)B, cfg) * 4 + 64);
        if (rc == KZG_OK) rc = s.offs.reserve(ctx, ((size_t)cfg.nb * B + 1) * 4);
        if (rc == KZG_OK) rc = s.block_sums.reserve(ctx, (size_t)sort_workspace_words() * 4);  // bin starts, chunk plan, fill counters, fine-pass table
        if (rc) return rc;
        HIP_TRY(ctx, hipMemset(s.block_sums.p, 0, (size_t)sort_workspace_zero_words() * 4));
        rc = s.pairs.reserve(ctx, (pairs ? pairs : 1) * 8);
        if (rc == KZG_OK) rc = s.recoded.reserve(ctx, (ctx->n * B ? ctx->n * B : 1) * 32);
        if (rc == KZG_OK) rc = s.sorted.reserve(ctx, (pairs ? pairs : 1) * 4);
        if (rc == KZG_OK) rc = s.buckets.reserve(ctx, (size_t)cfg.nb * B * kXyzzBytes);
        if (rc == KZG_OK) rc = s.part_a.reserve(ctx, (size_t)kMaxAccumLanes * kXyzzBytes);
        if (rc == KZG_OK) rc = s.part_b.reserve(ctx, (size_t)kMaxAccumLanes * kXyzzBytes);
        if (rc == KZG_OK) rc = s.pair_scratch.reserve(ctx, accumulate_pair_scratch_bytes(pairs));  // 0 without KZG_ACCUM_PAIRS=1
        if (rc == KZG_OK) rc = s.heavy_ws.reserve(ctx, heavy_workspace_bytes());
        if (rc == KZG_OK) rc = s.arena.reserve(ctx, ctx->arena_records * B * kXyzzBytes);
        if (rc == KZG_OK) rc = s.fin.reserve(ctx, ctx->final_records * B * kXyzzBytes);
        if (rc) return rc;
        s.kind = SLOT_IDLE;
    }
    ctx->slots_ready = true;
    return KZG_OK;
}

// builds levels 1..W-1 of the table from level 0 (already in table[0..n))
int build_tables(kzg_ctx* ctx, hipStream_t st, void* d_xyzz_tmp, void* d_prefix) {
    const size_t n = ctx->n;
    for (uint32_t j = 1; j < ctx->cfg.W; j++) {
        char* prev = (char*)ctx->table.p + (size_t)(j - 1) * n * kAffineBytes;
        char* next = (char*)ctx->table.p + (size_t)j * n * kAffineBytes;
        launch_table_window(st, prev, (uint32_t)n, ctx->cfg.level_bits, d_xyzz_tmp, d_prefix, next);
    }
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipStreamSynchronize(st));
    return KZG_OK;
}

// nothing of any job is in flight after this: the streams in the order a job passes through them
int drain_all(kzg_ctx* ctx) {
    for (hipStream_t st : {ctx->upload_stream, ctx->front_stream, ctx->heavy_stream, ctx->tail_stream})
        if (st) HIP_TRY(ctx, hipStreamSynchronize(st));
    return KZG_OK;
}

// the context gives up its SRS: nothing in flight, no table, n = 0 (the slots keep their workspaces for the next one)
static int srs_release(kzg_ctx* ctx) {
    ctx->slots_ready = false;
    int rc = drain_all(ctx);
    if (rc) return rc;
    for (auto& s : ctx->slots) s.kind = SLOT_IDLE;
    ctx->table.reset();
    ctx->fk20_B.reset();  // the FK20 cache holds transforms of the old SRS
    ctx->fk20_tab.reset();
    ctx->lag_table.reset();  // ... and the Lagrange basis is a transform of it: dropped, not rebuilt
    ctx->lag_n = 0;
    ctx->srs_gen++;
    ctx->n = 0;
    return KZG_OK;
}

int srs_prepare(kzg_ctx* ctx, size_t n) {
    if (n == 0 || n > 0x7fffffffu / 32) return KZG_ERR_INVALID_ARG;
    int rc = srs_release(ctx);
    if (rc) return rc;
    // The opt-in NAF recoding wants a 255-level table (engine.h); it may take up to 60 % of the HBM that is free
    // now (KZG_TABLE_GB overrides), otherwise the windowed recoding with its ~15 levels is used.
    size_t free_b = 0, total_b = 0;
    HIP_TRY(ctx, hipMemGetInfo(&free_b, &total_b));
    size_t budget = (size_t)((double)free_b * 0.6);
    if (const char* v = std::getenv("KZG_TABLE_GB")) budget = (size_t)(std::strtod(v, nullptr) * 1073741824.0);
    MsmConfig cfg = choose_msm_config(n, budget);
    if ((size_t)cfg.W * n >= 0x80000000ull) return KZG_ERR_INVALID_ARG;  // table index must fit 31 bits
    ctx->cfg = cfg;
    return ctx->table.reserve(ctx, (size_t)cfg.W * n * kAffineBytes);
}

// enqueue `batch` MSMs of n scalars each (polynomial p at d_scalars + p * stride scalars) on slot s: the sort on the
// front stream, the accumulation on the accumulation stream, the rest on the tail stream.  Leaves in s.end the stream the job
// ended on: whatever the caller enqueues behind the MSM (its `done` event) goes THERE, never on the front stream.
// basis: the window table the job reads, the monomial SRS when null.
struct MsmBasis {
    const void* table;  // W levels of `stride` affine records each
    uint32_t stride;
};
int enqueue_msm(kzg_ctx* ctx, Slot& s, const uint32_t* d_scalars, int is_mont, size_t n, int ev_base,
                uint32_t batch = 1, uint64_t stride = 0, const MsmBasis* basis = nullptr) {
    const MsmConfig cfg = ctx->cfg;
    const void* table = basis ? basis->table : ctx->table.p;
    const uint32_t table_stride = basis ? basis->stride : (uint32_t)ctx->n;
    const uint32_t nbt = cfg.nb * batch;  // polynomial-major bucket ids
    hipStream_t st = s.stream;
    s.end = st;
    if (s.timing) HIP_TRY(ctx, hipEventRecord(s.ev[ev_base], st));
    const bool header_zeroed = launch_bucket_sort(st, d_scalars, is_mont, (uint32_t)n, batch, stride, table_stride, cfg, s.cnt.dev(),
                       s.block_sums.dev(), s.pairs.dev<uint64_t>(), s.recoded.dev(), s.offs.dev(), s.sorted.dev(), (uint32_t*)s.heavy_ws.p);
    if (s.timing) {
        HIP_TRY(ctx, hipEventRecord(s.ev[ev_base + 1], st));
        HIP_TRY(ctx, hipEventRecord(s.ev[ev_base + 2], st));
    }
    bool alone = true;  // (this slot is still marked idle while its job is being enqueued)
    for (const auto& other : ctx->slots) alone = alone && (&other == &s || other.kind == SLOT_IDLE);
    const uint64_t max_refs = (uint64_t)n * cfg.max_digits * batch;
    const uint32_t lanes = accumulate_lanes(max_refs, alone);
    // reduction: Row / Col tree sums of every polynomial's bucket matrix, each split once more.
    // Vectors are polynomial-major ([p][index]); the final buffer holds four sections [p][len_k].
    const ReducePlan& P = ctx->plan;
    const uint32_t R = 1u << P.hi_bits, C = 1u << P.lo_bits, B = batch;
    char* row = (char*)s.arena.p;
    char* col = row + (size_t)R * B * kXyzzBytes;
    char* fin = (char*)s.fin.d;
    const uint32_t rl = 1u << P.row_lo, rh = 1u << P.row_hi, cl = 1u << P.col_lo, ch = 1u << P.col_hi;
    const TreeSumDesc stage1[2] = {
        {s.buckets.p, row, B * R, C, C, 1, B * R, 0},           // Row[p][hi] = sum_lo Bk[p][hi*C + lo]
        {s.buckets.p, col, B * C, R, 1, C, C, (uint64_t)cfg.nb}};  // Col[p][lo] = sum_hi Bk[p][hi*C + lo]
    const TreeSumDesc stage2[4] = {
        {row, fin + (size_t)P.off_r2row * B * kXyzzBytes, B * rh, rl, rl, 1, rh, R},
        {row, fin + (size_t)P.off_c2row * B * kXyzzBytes, B * rl, rh, 1, rl, rl, R},
        {col, fin + (size_t)P.off_r2col * B * kXyzzBytes, B * ch, cl, cl, 1, ch, C},
        {col, fin + (size_t)P.off_c2col * B * kXyzzBytes, B * cl, ch, 1, cl, cl, C}};
    if (!header_zeroed) HIP_TRY(ctx, hipMemsetAsync(s.heavy_ws.p, 0, kHeavyHeaderBytes, st));  // long-bucket counters, phase counters
    if (max_refs <= kTinyRefs && !ctx->small_msm_off) {
        // Small jobs are chains of dependent additions on a nearly empty chip: everything from here to the copy back
        // in ONE launch on the front stream (msm_finalize.hip: k_small_msm), no bucket memset, no stream hand-over.
        if (s.timing) HIP_TRY(ctx, hipEventRecord(s.ev[ev_base + 3], st));
        launch_small_msm(st, table, s.sorted.dev(), s.offs.dev(), nbt, lanes, max_refs, s.buckets.p, s.part_a.p, s.part_b.p,
                         s.heavy_ws.p, s.small.dev() + 26, stage1, stage2, ctx->small_lds_bytes);
        if (s.timing) HIP_TRY(ctx, hipEventRecord(s.ev[ev_base + 4], st));
    } else {
        // hand over to the accumulation stream and on to the tail stream (each hand-over costs ~12 us: not when no other
        // slot has work whose accumulation this one could collide with -- the whole job then stays on the front stream)
        const bool hand_over = !alone;
        hipStream_t hs = hand_over ? ctx->heavy_stream : st;
        if (hand_over) {
            HIP_TRY(ctx, hipEventRecord(s.sorted_ev, st));
            HIP_TRY(ctx, hipStreamWaitEvent(hs, s.sorted_ev, 0));
        }
        if (s.timing) HIP_TRY(ctx, hipEventRecord(s.ev[ev_base + 3], hs));
        launch_bucket_accumulate(hs, table, s.sorted.dev(), s.offs.dev(), nbt, lanes, s.buckets.p, s.part_a.p, s.part_b.p,
                                 ctx->accum_lds_bytes, s.pair_scratch.p, max_refs,
                                 (char*)s.heavy_ws.p + kAccumClockOffset);
        if (s.timing) HIP_TRY(ctx, hipEventRecord(s.ev[ev_base + 4], hs));
        if (hand_over) {
            HIP_TRY(ctx, hipEventRecord(s.accum_ev, hs));
            st = s.end = ctx->tail_stream;
            HIP_TRY(ctx, hipStreamWaitEvent(st, s.accum_ev, 0));
        }
        launch_bucket_finalize(st, s.offs.dev(), nbt, lanes, s.part_a.p, s.part_b.p, s.buckets.p, s.heavy_ws.p, s.small.dev() + 26,
                               finalize_group_size(nbt));
        // (Rounds 1-2 put a gate kernel here that deferred the reduction trees to the tail of the next slot's
        // accumulation: worth 20 % with round 1's 206-VGPR accumulation kernel, beside which the trees could become
        // resident; the trees (243-258 VGPRs) cannot start beside round 3's accumulation kernel whatever the stream
        // order says, and with or without a gate -- LDS-sized or a device-side count of running workgroups -- round 3
        // measured 409 / 384 against 408 / 383 and 414 / 386 against 415 / 386 commitments / proofs per second.  Retired.)
        launch_tree_sums_two_stage(st, stage1, 2, stage2, 4, (uint32_t*)s.heavy_ws.p + 64, alone);
    }
    if (s.timing) HIP_TRY(ctx, hipEventRecord(s.ev[ev_base + 5], st));
    HIP_TRY(ctx, hipGetLastError());
    return KZG_OK;
}

// host tail.  With V indexed by u = u1 * 2^lo + u0:  sum_u u V_u = 2^lo * wsum(R2) + wsum(C2), where
// R2[u1] = sum_u0 V, C2[u0] = sum_u1 V and wsum(P) = sum_v v * P_v (running sums, <= 32 entries).
hf::PX host_wsum(const uint64_t* recs, uint32_t len) {
    hf::PX run = hf::px_inf(), acc = hf::px_inf();
    for (uint32_t v = len; v-- > 1;) {
        run = hf::px_add(run, hf::px_from_record(recs + (size_t)v * kXyzzWords64));
        acc = hf::px_add(acc, run);
    }
    return acc;
}
hf::PX host_shift(hf::PX p, uint32_t k) {
    for (uint32_t i = 0; i < k; i++) p = hf::px_double(p);
    return p;
}
hf::P1 finish_msm(const kzg_ctx* ctx, const Slot& s, uint32_t p = 0, uint32_t batch = 1) {
    const ReducePlan& P = ctx->plan;
    const uint64_t* f = s.fin.host<uint64_t>();
    // section k of the final buffer is [batch][len_k]: polynomial p's block starts at off_k*batch + p*len_k
    auto at = [&](uint32_t off, uint32_t len) { return f + ((size_t)off * batch + (size_t)p * len) * kXyzzWords64; };
    const uint32_t rh = 1u << P.row_hi, rl = 1u << P.row_lo, ch = 1u << P.col_hi, cl = 1u << P.col_lo;
    // W(Row) = 2^row_lo * wsum(R2row) + wsum(C2row);  W(Col) likewise
    hf::PX w_row = hf::px_add(host_shift(host_wsum(at(P.off_r2row, rh), rh), P.row_lo), host_wsum(at(P.off_c2row, rl), rl));
    hf::PX w_col = hf::px_add(host_shift(host_wsum(at(P.off_r2col, ch), ch), P.col_lo), host_wsum(at(P.off_c2col, cl), cl));
    // sum_b b B_b = C * W(Row) + W(Col);  sum_b B_b = sum of R2row.
    // Bucket b weighs b + 1 (windows: digit magnitude) or 2b + 1 (NAF: odd digits only).
    hf::PX total = hf::px_add(host_shift(w_row, P.lo_bits), w_col);
    if (ctx->cfg.recode == kRecodeNaf) total = hf::px_double(total);
    const uint64_t* r2 = at(P.off_r2row, rh);
    for (uint32_t k = 0; k < rh; k++) total = hf::px_add(total, hf::px_from_record(r2 + (size_t)k * kXyzzWords64));
    // a kid of a range-split multi-device context hands its partial sum on as it is (Jacobian, two products); the
    // parent pays the one inversion after adding the K partials (multi.hip)
    return ctx->raw_partials ? hf::px_to_jacobian(total) : hf::px_normalize(total);
}

void write_p1(uint64_t out[18], const hf::P1& p) { std::memcpy(out, &p, sizeof p); }

// EVERY job: accumulate_ms is the accumulation kernel's own duration -- first wave in to last wave out on the constant
// 100 MHz clock, stamped by the kernel and passed on by the finalisation (small[28..31]; the one-launch path of
// small jobs leaves it 0) -- and `references` its number of mixed additions: no stream event is involved.  Timed jobs
// (kzg_set_timing) also get the HIP-event spans; accumulate_events_ms is the bracket around the same launch on its
// stream, which holds the time the launch waited for the chip as well.
void fill_device_times(Slot& s) {
    s.times.references = s.small.host()[26];
    const uint64_t not_start = (uint64_t)s.small.host()[28] | ((uint64_t)s.small.host()[29] << 32);
    const uint64_t end = (uint64_t)s.small.host()[30] | ((uint64_t)s.small.host()[31] << 32);
    if (not_start != 0 && end > ~not_start) s.times.accumulate_ms = (float)((double)(end - ~not_start) * 1e-5);  // 10 ns ticks
}
void fill_accumulate_times(Slot& s) {  // timed jobs, after fill_device_times
    float ms = 0;
    (void)hipEventElapsedTime(&ms, s.ev[3], s.ev[4]);
    s.times.accumulate_events_ms = ms;
    if (s.times.accumulate_ms == 0) s.times.accumulate_ms = ms;
}

// ---- slot ownership of the synchronous host-pointer entry points (all of these with ctx->mu held) ------------------
void slot_idle(kzg_ctx* ctx, Slot& s) {
    s.kind = SLOT_IDLE;
    ctx->slot_cv.notify_all();
}
// an idle slot, marked SLOT_RESERVED for the caller; -1 when none is free and (block == false, or every busy slot
// belongs to an explicit submit whose owner may be this very thread: waiting for it could never end -> KZG_ERR_BUSY)
int reserve_slot(kzg_ctx* ctx, std::unique_lock<std::mutex>& lk, bool block) {
    for (;;) {
        for (int i = 0; i < kNumSlots; i++)
            if (ctx->slots[i].kind == SLOT_IDLE) {
                ctx->slots[i].kind = SLOT_RESERVED;
                ctx->sync_owned++;
                return i;
            }
        if (!block || ctx->sync_owned == 0) return -1;
        ctx->slot_cv.wait(lk);
    }
}
void release_owned(kzg_ctx* ctx, int slot) {
    if (ctx->slots[slot].kind == SLOT_RESERVED) ctx->slots[slot].kind = SLOT_IDLE;
    ctx->sync_owned--;
    ctx->slot_cv.notify_all();
}
struct SlotLease {  // declared after the lock it lives under: released first
    kzg_ctx* ctx;
    int slot;
    ~SlotLease() { if (slot >= 0) release_owned(ctx, slot); }
};
// SRS replacement and workspace resizing wait until no synchronous call is between its steps
void quiesce(kzg_ctx* ctx, std::unique_lock<std::mutex>& lk) {
    while (ctx->sync_owned > 0) ctx->slot_cv.wait(lk);
}

bool host_tail_nonzero(const uint64_t* coeffs, size_t from, size_t n) {
    for (size_t i = from; i < n; i++)
        if (coeffs[4 * i] | coeffs[4 * i + 1] | coeffs[4 * i + 2] | coeffs[4 * i + 3]) return true;
    return false;
}

// ---- multiproofs (kzg_open_points and friends) ---------------------------------------------------------------------
// 1 <= k <= KZG_MAX_OPEN_POINTS and pairwise-distinct points; ws receives w_i = 1 / prod_{j != i} (z_i - z_j)
int points_weights(kzg_ctx* ctx, const uint64_t* zs, size_t k, uint64_t* ws /* 4 k */) {
    if (k < 1 || k > KZG_MAX_OPEN_POINTS) {
        ctx->last_error = "multiproof: k must be in [1, KZG_MAX_OPEN_POINTS]";
        return KZG_ERR_INVALID_ARG;
    }
    hf::Fr z[KZG_MAX_OPEN_POINTS], w[KZG_MAX_OPEN_POINTS];
    std::memcpy(z, zs, 32 * k);
    if (!hf::fr_point_weights(z, k, w)) {
        ctx->last_error = "multiproof: two of the points are equal";
        return KZG_ERR_INVALID_ARG;
    }
    std::memcpy(ws, w, 32 * k);
    return KZG_OK;
}
// the slot's multiproof buffers for k roots over n coefficients (slot basics already there)
int ensure_points(kzg_ctx* ctx, Slot& s, size_t n, size_t k) {
    int rc = s.roots.reserve(ctx, KZG_MAX_OPEN_POINTS * points_root_bytes());
    if (rc == KZG_OK) rc = s.pvals.reserve(ctx, KZG_MAX_OPEN_POINTS * 32);
    if (rc == KZG_OK) rc = s.pblock.reserve(ctx, k * poly_block_words((uint32_t)(n ? n : 1)) * 4, s.stream);
    return rc;
}
// where the scan of a multiproof leaves P(z_i): the single-root kernels (k == 1) write the slot's flag words
const uint32_t* points_values(const Slot& s, size_t k) { return k == 1 ? s.small.host() + 8 : s.pvals.host(); }
// enqueues the scan of P at the k points on the front stream: q[0 .. nq) to s.q when want_q, the values as above.
// k == 1 takes the single-root kernels unchanged (w_0 = 1), so its proofs are kzg_open's bit for bit.
int enqueue_points_scan(kzg_ctx* ctx, Slot& s, const uint32_t* d_coeffs, size_t n, const uint64_t* zs, const uint64_t* ws,
                        size_t k, size_t nq, bool want_q) {
    std::memset(s.small.host(), 0, 64 * 4);  // (the slot holds no job in flight: nothing writes them now)
    std::memset(s.pvals.host(), 0, 32 * k);
    if (n == 0) return KZG_OK;           // P = 0: every value is zero
    if (k == 1) {
        uint32_t zw[8];
        std::memcpy(zw, zs, 32);
        uint32_t* q = want_q && n > 1 ? s.q.dev() : nullptr;
        if (!launch_quotient_single(s.stream, d_coeffs, (uint32_t)n, zw, q, s.small.dev())) {
            PolyScratch sc{s.chunk.dev(), s.block.dev(), s.small.dev(), s.small.dev() + 8};
            launch_quotient(s.stream, d_coeffs, (uint32_t)n, zw, q, sc);
        }
    } else {
        points_fill_roots(s.roots.h, zs, ws, (uint32_t)k, (uint32_t)n);
        HIP_TRY(ctx, hipMemcpyAsync(s.roots.d, s.roots.h, k * points_root_bytes(), hipMemcpyHostToDevice, s.stream));
        launch_quotient_points(s.stream, d_coeffs, (uint32_t)n, s.roots.d, (uint32_t)k, want_q ? s.q.dev() : nullptr, (uint32_t)nq,
                               s.pblock.dev(), s.pvals.dev());
    }
    HIP_TRY(ctx, hipGetLastError());
    return KZG_OK;
}

}  // namespace

// a tiny kernel for the device-pointer entry points: any non-zero Fr in [from, n)?
__global__ void k_tail_nonzero(const uint32_t* __restrict__ c, uint64_t from, uint64_t n, uint32_t* __restrict__ flag) {
    uint64_t i = from + (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint4* p = reinterpret_cast<const uint4*>(c) + 2 * i;
    uint4 a = p[0], b = p[1];
    if (a.x | a.y | a.z | a.w | b.x | b.y | b.z | b.w) *flag = 1u;  // (host-mapped word: plain store, every writer stores 1)
}

// asynchronous / device-pointer entry points belong to ONE device: refused on a multi-device context
#define KZG_SINGLE_DEVICE_ONLY(ctx)                                                                        \
    do {                                                                                                     \
        if ((ctx) && (ctx)->multi) {                                                                         \
            (ctx)->last_error = "this entry point takes a single-device context (kzg_ctx_create)";           \
            return KZG_ERR_INVALID_ARG;                                                                      \
        }                                                                                                    \
    } while (0)

extern "C" {

const char* kzg_strerror(int status) {
    switch (status) {
        case KZG_OK: return "ok";
        case KZG_ERR_DEGREE_TOO_HIGH:
            return "Setup does not allow for commitment generation of the polynomial. The polynomial degree is too high.";
        case KZG_ERR_CONSTANT_POLY: return "Unable to divide a constant polynomial";
        case KZG_ERR_REMAINDER:
            return "[divide_by_root] Fail to divide the polynomial by a root, constant terms do not add up";
        case KZG_ERR_INVALID_ARG: return "invalid argument";
        case KZG_ERR_NO_DEVICE: return "no HIP device available (this library has no CPU path)";
        case KZG_ERR_HIP: return "HIP runtime error";
        case KZG_ERR_NO_SRS: return "no SRS loaded";
        case KZG_ERR_BUSY: return "slot busy";
        default: return "unknown status";
    }
}

const char* kzg_last_error(const kzg_ctx* ctx) {
    if (!ctx) return "";
    if (ctx->multi && ctx->last_error.empty()) return multi_last_error(ctx->multi);
    return ctx->last_error.c_str();
}

int kzg_ctx_create_multi_ex(const int* devices, int ndev, unsigned flags, kzg_ctx** out) {
    if (!out) return KZG_ERR_INVALID_ARG;
    *out = nullptr;
    if (!devices || ndev <= 0 || (flags & ~(unsigned)KZG_MULTI_REPLICATE_SRS)) return KZG_ERR_INVALID_ARG;
    kzg::MultiState* m = nullptr;
    std::string err;
    int rc = multi_create(devices, ndev, (flags & KZG_MULTI_REPLICATE_SRS) ? kMultiReplicate : kMultiRange, &m, err);
    if (rc != KZG_OK) return rc;
    kzg_ctx* ctx = new kzg_ctx();
    ctx->multi = m;
    ctx->device = devices[0];
    *out = ctx;
    return KZG_OK;
}
int kzg_ctx_create_multi(const int* devices, int ndev, kzg_ctx** out) { return kzg_ctx_create_multi_ex(devices, ndev, 0u, out); }
int kzg_abi_version(void) { return KZG_ABI_VERSION; }
int kzg_num_devices(const kzg_ctx* ctx) { return !ctx ? 0 : (ctx->multi ? multi_num_devices(ctx->multi) : 1); }
uint64_t kzg_rccl_exchanges(const kzg_ctx* ctx) { return (ctx && ctx->multi) ? multi_rccl_exchanges(ctx->multi) : 0; }

int kzg_ctx_create(int device, kzg_ctx** out) {
    if (!out) return KZG_ERR_INVALID_ARG;
    *out = nullptr;
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) return KZG_ERR_NO_DEVICE;
    if (device < 0 || device >= count) return KZG_ERR_NO_DEVICE;
    if (hipSetDevice(device) != hipSuccess) return KZG_ERR_NO_DEVICE;
    kzg_ctx* ctx = new kzg_ctx();
    ctx->device = device;
    if (const char* v = std::getenv("KZG_ACCUM_LDS_KB")) ctx->accum_lds_bytes = (uint32_t)std::atoi(v) * 1024u;
    if (const char* v = std::getenv("KZG_SMALL_MSM")) ctx->small_msm_off = std::atoi(v) == 0;
    if (const char* v = std::getenv("KZG_PQ_WS_KB")) {  // never above the default: the passes only get smaller
        const long kb = std::atol(v);
        ctx->pq_ws_budget = kb < 0 ? 0 : (kb > (1l << 20) ? (size_t)1 << 30 : (size_t)kb * 1024);
    }
    if (const char* v = std::getenv("KZG_HOST_TRACE")) ctx->host_trace = std::atoi(v) != 0;
    if (hipFuncSetAttribute(small_msm_kernel(), hipFuncAttributeMaxDynamicSharedMemorySize, (int)small_msm_lds_bytes()) == hipSuccess)
        ctx->small_lds_bytes = small_msm_lds_bytes();
    else
        (void)hipGetLastError();  // stays at 48 KiB: two workgroups may then share a CU (slower, not wrong)
    if (!poly_prepare_device() || !points_prepare_device() || !sets_prepare_device()) {
        delete ctx;
        return KZG_ERR_HIP;  // the quotient kernels could not be launched on this device
    }
    *out = ctx;
    return KZG_OK;
}

void kzg_ctx_destroy(kzg_ctx* ctx) {
    if (!ctx) return;
    if (ctx->multi) {
        multi_destroy(ctx->multi);
        delete ctx;
        return;
    }
    hipSetDevice(ctx->device);
    if (ctx->host_trace && ctx->trace_calls.load()) {
        const double k = 1e-3 / (double)ctx->trace_calls.load();
        std::fprintf(stderr, "[kzg host trace] %llu kzg_commit calls, us per call: wait-for-slot %.1f upload %.1f submit %.1f device %.1f collect %.1f\n",
                     (unsigned long long)ctx->trace_calls.load(), k * ctx->trace_ns[0].load(), k * ctx->trace_ns[1].load(),
                     k * ctx->trace_ns[2].load(), k * ctx->trace_ns[3].load(), k * ctx->trace_ns[4].load());
    }
    // What has an order: the streams are waited for before any buffer goes and destroyed here, once (the slots only
    // hold the front stream's handle).  `delete` then frees the slots' buffers (members) and after them each slot's events
    // (its base, SlotQueue), between the context's own buffers.
    for (hipStream_t st : {ctx->upload_stream, ctx->front_stream, ctx->heavy_stream, ctx->tail_stream})
        if (st) hipStreamSynchronize(st);
    for (hipStream_t st : {ctx->upload_stream, ctx->front_stream, ctx->heavy_stream, ctx->tail_stream})
        if (st) hipStreamDestroy(st);
    for (kzg_circuit* c : ctx->circuits) delete c;  // (nothing runs any more: the streams were waited for)
    delete ctx;
}

size_t kzg_srs_len(const kzg_ctx* ctx) { return !ctx ? 0 : (ctx->multi ? multi_srs_len(ctx->multi) : ctx->n); }
int kzg_num_slots(const kzg_ctx*) { return kNumSlots; }

int kzg_msm_config(const kzg_ctx* ctx, int* digit_bits, int* table_levels, size_t* num_buckets, int* recoding) {
    if (ctx && ctx->multi)  // the first slice's configuration (all slices have the same length up to one point)
        return kzg_msm_config(multi_kid(ctx->multi, 0), digit_bits, table_levels, num_buckets, recoding);
    if (!ctx || !ctx->n) return KZG_ERR_NO_SRS;
    if (digit_bits) *digit_bits = (int)ctx->cfg.c;
    if (table_levels) *table_levels = (int)ctx->cfg.W;
    if (num_buckets) *num_buckets = ctx->cfg.nb;
    if (recoding) *recoding = (int)ctx->cfg.recode;
    return KZG_OK;
}

int kzg_srs_load_g1(kzg_ctx* ctx, const void* first_g1, size_t stride, size_t n) {
    if (!ctx || !first_g1 || stride < 144) return KZG_ERR_INVALID_ARG;
    if (ctx->multi) {
        std::lock_guard<std::mutex> lkm(ctx->mu);
        ctx->last_error.clear();
        return n ? multi_srs_load(ctx->multi, first_g1, stride, n) : KZG_ERR_INVALID_ARG;
    }
    std::unique_lock<std::mutex> lk(ctx->mu);
    quiesce(ctx, lk);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    int rc = srs_prepare(ctx, n);
    if (rc) return rc;
    // gather the strided blst_p1 values, upload, normalise to affine = window 0
    std::vector<uint64_t> packed(n * 18);
    for (size_t i = 0; i < n; i++) std::memcpy(&packed[i * 18], (const char*)first_g1 + i * stride, 144);
    DevBuf d_jac, d_prefix, d_xyzz;
    HIP_TRY(ctx, hipMalloc(&d_jac.p, n * 144));
    HIP_TRY(ctx, hipMalloc(&d_prefix.p, n * 64));
    HIP_TRY(ctx, hipMalloc(&d_xyzz.p, n * kXyzzBytes));
    TmpStream st;
    HIP_TRY(ctx, hipStreamCreateWithFlags(&st.s, hipStreamNonBlocking));
    HIP_TRY(ctx, hipMemcpyAsync(d_jac.p, packed.data(), n * 144, hipMemcpyHostToDevice, st.s));
    ctx->n = n;
    launch_jacobian_to_affine(st.s, d_jac.p, (uint32_t)n, ctx->table.p, d_prefix.p);
    rc = build_tables(ctx, st.s, d_xyzz.p, d_prefix.p);
    if (rc) {
        ctx->n = 0;
        return rc;
    }
    return setup_slots(ctx);
}

int kzg_srs_generate_g1(kzg_ctx* ctx, const uint8_t secret_be[32], uint64_t first, size_t n) {
    if (!ctx || !secret_be) return KZG_ERR_INVALID_ARG;
    if (ctx->multi) {
        std::lock_guard<std::mutex> lkm(ctx->mu);
        ctx->last_error.clear();
        return n ? multi_srs_generate(ctx->multi, secret_be, first, n) : KZG_ERR_INVALID_ARG;
    }
    std::unique_lock<std::mutex> lk(ctx->mu);
    quiesce(ctx, lk);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    int rc = srs_prepare(ctx, n);
    if (rc) return rc;
    uint32_t raw[8];
    for (int w = 0; w < 8; w++) {
        // big-endian bytes -> little-endian 32-bit words (reference src/trusted_setup.rs:24)
        const uint8_t* b = secret_be + 28 - 4 * w;
        raw[w] = ((uint32_t)b[0] << 24) | ((uint32_t)b[1] << 16) | ((uint32_t)b[2] << 8) | (uint32_t)b[3];
    }
    size_t tmp_records = n > 32 * 255 ? n : 32 * 255;
    DevBuf d_gtable, d_prefix, d_xyzz;
    HIP_TRY(ctx, hipMalloc(&d_gtable.p, srs_gtable_bytes()));
    HIP_TRY(ctx, hipMalloc(&d_prefix.p, tmp_records * 64));
    HIP_TRY(ctx, hipMalloc(&d_xyzz.p, tmp_records * kXyzzBytes));
    TmpStream st;
    HIP_TRY(ctx, hipStreamCreateWithFlags(&st.s, hipStreamNonBlocking));
    ctx->n = n;
    launch_srs_generate(st.s, raw, first, (uint32_t)n, d_gtable.p, d_xyzz.p, d_prefix.p, ctx->table.p);
    rc = build_tables(ctx, st.s, d_xyzz.p, d_prefix.p);
    if (rc) {
        ctx->n = 0;
        return rc;
    }
    return setup_slots(ctx);
}

// level 0 is in table (builder's form): build the other levels, convert, size the slots
static int finish_srs_from_level0(kzg_ctx* ctx, hipStream_t st, size_t n) {
    DevBuf d_prefix, d_xyzz;
    HIP_TRY(ctx, hipMalloc(&d_prefix.p, n * 64));
    HIP_TRY(ctx, hipMalloc(&d_xyzz.p, n * kXyzzBytes));
    ctx->n = n;
    int rc = build_tables(ctx, st, d_xyzz.p, d_prefix.p);
    if (rc) {
        ctx->n = 0;
        return rc;
    }
    return setup_slots(ctx);
}

int kzg_srs_load_affine(kzg_ctx* ctx, const void* affine_xy, size_t n) {
    if (!ctx || !affine_xy || !n) return KZG_ERR_INVALID_ARG;
    std::unique_lock<std::mutex> lk(ctx->mu);
    if (ctx->multi) {
        ctx->last_error.clear();
        return multi_srs_load_affine(ctx->multi, affine_xy, n);
    }
    quiesce(ctx, lk);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    int rc = srs_prepare(ctx, n);
    if (rc) return rc;
    DevBuf d_in;
    HIP_TRY(ctx, hipMalloc(&d_in.p, n * 96));
    TmpStream st;
    HIP_TRY(ctx, hipStreamCreateWithFlags(&st.s, hipStreamNonBlocking));
    HIP_TRY(ctx, hipMemcpyAsync(d_in.p, affine_xy, n * 96, hipMemcpyHostToDevice, st.s));
    launch_affine96_to_table(st.s, d_in.p, (uint32_t)n, ctx->table.p);
    return finish_srs_from_level0(ctx, st.s, n);
}

int kzg_srs_load_compressed(kzg_ctx* ctx, const uint8_t* compressed, size_t n, size_t* bad_index) {
    if (!ctx || !compressed || !n) return KZG_ERR_INVALID_ARG;
    if (bad_index) *bad_index = (size_t)-1;
    std::unique_lock<std::mutex> lk(ctx->mu);
    if (ctx->multi) {
        ctx->last_error.clear();
        return multi_srs_load_compressed(ctx->multi, compressed, n, bad_index);
    }
    quiesce(ctx, lk);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    int rc = srs_prepare(ctx, n);
    if (rc) return rc;
    DevBuf d_in, d_status;
    HIP_TRY(ctx, hipMalloc(&d_in.p, n * 48));
    HIP_TRY(ctx, hipMalloc(&d_status.p, 4));
    TmpStream st;
    HIP_TRY(ctx, hipStreamCreateWithFlags(&st.s, hipStreamNonBlocking));
    HIP_TRY(ctx, hipMemcpyAsync(d_in.p, compressed, n * 48, hipMemcpyHostToDevice, st.s));
    HIP_TRY(ctx, hipMemsetAsync(d_status.p, 0xff, 4, st.s));
    launch_uncompress(st.s, d_in.p, (uint32_t)n, ctx->table.p, (uint32_t*)d_status.p);
    uint32_t status = 0;
    HIP_TRY(ctx, hipMemcpyAsync(&status, d_status.p, 4, hipMemcpyDeviceToHost, st.s));
    HIP_TRY(ctx, hipStreamSynchronize(st.s));
    if (status != 0xffffffffu) {  // a malformed point (not compressed form, x >= p, not on the curve): as blst_p1_uncompress
        if (bad_index) *bad_index = status - 1;
        ctx->last_error = "compressed point " + std::to_string(status - 1) + " is malformed";
        ctx->table.reset();
        return KZG_ERR_INVALID_ARG;
    }
    return finish_srs_from_level0(ctx, st.s, n);
}

// ---- binary SRS cache: 128-byte header + n x 96-byte affine points ----------------------------------------------
namespace {
struct SrsFileHeader {
    char magic[8];        // "KZGSRS1"
    uint64_t n;
    uint8_t first[48];    // compressed encodings of the first and the last point: fingerprint of the content
    uint8_t last[48];
    uint8_t reserved[16];
};
static_assert(sizeof(SrsFileHeader) == 128, "header layout");
const char kSrsMagic[8] = {'K', 'Z', 'G', 'S', 'R', 'S', '1', 0};

void affine96_compress(const uint64_t* xy, uint8_t out[48]) {
    hf::P1 p;
    std::memcpy(&p.x, xy, 48);
    std::memcpy(&p.y, xy + 6, 48);
    bool inf = true;
    for (int i = 0; i < 12; i++) inf = inf && xy[i] == 0;
    std::memset(&p.z, 0, 48);
    if (!inf) p.z = hf::kOne;
    hf::p1_compress(out, p);
}
}  // namespace

int kzg_srs_save(kzg_ctx* ctx, const char* path) {
    if (!ctx || !path) return KZG_ERR_INVALID_ARG;
    const size_t n = kzg_srs_len(ctx);
    if (!n) return KZG_ERR_NO_SRS;
    FILE* f = std::fopen(path, "wb");
    if (!f) return KZG_ERR_INVALID_ARG;
    SrsFileHeader h;
    std::memset(&h, 0, sizeof h);
    std::memcpy(h.magic, kSrsMagic, 8);
    h.n = n;
    bool ok = std::fwrite(&h, sizeof h, 1, f) == 1;
    const size_t chunk = 1 << 16;
    std::vector<uint64_t> p1(chunk * 18), xy(chunk * 12);
    for (size_t at = 0; at < n && ok; at += chunk) {
        const size_t take = n - at < chunk ? n - at : chunk;
        int rc = kzg_srs_read_g1(ctx, at, take, p1.data());
        if (rc != KZG_OK) {
            std::fclose(f);
            return rc;
        }
        for (size_t i = 0; i < take; i++) std::memcpy(&xy[12 * i], &p1[18 * i], 96);  // x, y of the affine blst_p1; infinity reads (0, 0)
        if (at == 0) affine96_compress(xy.data(), h.first);
        if (at + take == n) affine96_compress(&xy[12 * (take - 1)], h.last);
        ok = std::fwrite(xy.data(), 96, take, f) == take;
    }
    ok = ok && std::fseek(f, 0, SEEK_SET) == 0 && std::fwrite(&h, sizeof h, 1, f) == 1;
    ok = (std::fclose(f) == 0) && ok;
    return ok ? KZG_OK : KZG_ERR_INVALID_ARG;
}

// on-curve check of the loaded points (host, spread over the cores): a corrupted cache must not commit silently
static bool affine96_all_on_curve(const uint64_t* xy, size_t n, size_t* bad) {
    size_t nthreads = std::thread::hardware_concurrency();
    if (nthreads == 0) nthreads = 1;
    if (nthreads > 16) nthreads = 16;
    if (nthreads > n / 4096 + 1) nthreads = n / 4096 + 1;
    std::vector<size_t> first_bad(nthreads, (size_t)-1);
    hf::Fp four = hf::kOne + hf::kOne;
    four = four + four;
    auto work = [&](size_t t) {
        for (size_t i = t; i < n; i += nthreads) {
            hf::Fp x, y;
            std::memcpy(&x, xy + 12 * i, 48);
            std::memcpy(&y, xy + 12 * i + 6, 48);
            if (x.is_zero() && y.is_zero()) continue;  // infinity
            const bool ok = hf::geq(hf::kP, x) && !(x == hf::kP) && hf::geq(hf::kP, y) && !(y == hf::kP) &&
                            hf::sqr(y) == hf::sqr(x) * x + four;
            if (!ok) {
                first_bad[t] = i;
                return;
            }
        }
    };
    std::vector<std::thread> pool;
    for (size_t t = 1; t < nthreads; t++) pool.emplace_back(work, t);
    work(0);
    for (auto& th : pool) th.join();
    size_t worst = (size_t)-1;
    for (size_t v : first_bad) worst = v < worst ? v : worst;
    if (bad) *bad = worst;
    return worst == (size_t)-1;
}

int kzg_srs_load_file(kzg_ctx* ctx, const char* path) {
    if (!ctx || !path) return KZG_ERR_INVALID_ARG;
    auto fail = [&](const std::string& why) {
        std::lock_guard<std::mutex> lk(ctx->mu);
        ctx->last_error = why;
        return (int)KZG_ERR_INVALID_ARG;
    };
    FILE* f = std::fopen(path, "rb");
    if (!f) return fail("cannot open the SRS file");
    SrsFileHeader h;
    bool ok = std::fread(&h, sizeof h, 1, f) == 1 && std::memcmp(h.magic, kSrsMagic, 8) == 0 && h.n > 0 && h.n <= 0x7fffffffu / 32;
    if (ok) {  // the header's n is trusted only as far as the file is that long
        ok = std::fseek(f, 0, SEEK_END) == 0;
        const long end = ok ? std::ftell(f) : -1;
        ok = ok && end >= 0 && (uint64_t)end == 128ull + 96ull * h.n && std::fseek(f, 128, SEEK_SET) == 0;
    }
    std::vector<uint64_t> xy;
    if (ok) {
        try {
            xy.resize((size_t)h.n * 12);
        } catch (const std::bad_alloc&) {  // nothing may unwind through the C-ABI
            std::fclose(f);
            return fail("out of host memory for the SRS file");
        }
        ok = std::fread(xy.data(), 96, h.n, f) == h.n;
    }
    std::fclose(f);
    if (ok) {  // fingerprint: first and last point as the header recorded them
        uint8_t a[48], b[48];
        affine96_compress(xy.data(), a);
        affine96_compress(&xy[12 * ((size_t)h.n - 1)], b);
        ok = std::memcmp(a, h.first, 48) == 0 && std::memcmp(b, h.last, 48) == 0;
    }
    if (!ok) return fail("not a KZGSRS1 file, truncated, or its fingerprint does not match its content");
    size_t bad = 0;
    if (!affine96_all_on_curve(xy.data(), (size_t)h.n, &bad)) return fail("SRS file: point " + std::to_string(bad) + " is not on the curve");
    return kzg_srs_load_affine(ctx, xy.data(), (size_t)h.n);
}

int kzg_srs_read_g1(kzg_ctx* ctx, size_t index, size_t count, uint64_t* out_p1) {
    if (!ctx || !out_p1) return KZG_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(ctx->mu);
    if (ctx->multi) return multi_srs_len(ctx->multi) ? multi_srs_read(ctx->multi, index, count, out_p1) : KZG_ERR_NO_SRS;
    if (!ctx->n) return KZG_ERR_NO_SRS;
    if (index > ctx->n || count > ctx->n - index) return KZG_ERR_INVALID_ARG;
    if (!count) return KZG_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    DevBuf d_p1;
    HIP_TRY(ctx, hipMalloc(&d_p1.p, count * 144));
    hipStream_t st = ctx->slots[0].stream;
    launch_affine_to_p1(st, (const char*)ctx->table.p + index * kAffineBytes, (uint32_t)count, d_p1.p);
    HIP_TRY(ctx, hipMemcpyAsync(out_p1, d_p1.p, count * 144, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    return KZG_OK;
}

// ---- submit / wait ---------------------------------------------------------------------------

// the held Lagrange basis as an MSM basis when it is the one of n points (ctx->mu held)
static bool lagrange_basis(const kzg_ctx* ctx, size_t n, MsmBasis* out) {
    if (!ctx->lag_table.p || ctx->lag_n != n) return false;
    *out = MsmBasis{ctx->lag_table.p, (uint32_t)ctx->lag_n};
    return true;
}

// owned: the caller holds the slot through reserve_slot (SLOT_RESERVED) instead of finding it idle
// basis: the table of exactly n points (n <= ctx->n) the MSM reads instead of the SRS -- the scalars are n values over its domain
static int submit_commit_locked(kzg_ctx* ctx, int slot, const uint32_t* d_scalars, int is_mont, size_t n,
                                bool tail_already_checked, bool owned = false, const MsmBasis* basis = nullptr) {
    if (!ctx->n || !ctx->slots_ready) return KZG_ERR_NO_SRS;
    if (basis && (basis->stride != n || n > ctx->n)) return KZG_ERR_INVALID_ARG;
    if (slot < 0 || slot >= kNumSlots) return KZG_ERR_INVALID_ARG;
    Slot& s = ctx->slots[slot];
    if (s.kind != (owned ? SLOT_RESERVED : SLOT_IDLE)) return KZG_ERR_BUSY;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    s.timing = ctx->timing;
    s.end = s.stream;
    s.has_quotient = false;
    s.job_n = n;
    s.job_batch = 1;
    s.tail_checked = tail_already_checked;
    std::memset(&s.times, 0, sizeof s.times);
    size_t n_msm = n < ctx->n ? n : ctx->n;
    std::memset(s.small.host(), 0, 64 * 4);  // (the slot is idle: nothing in flight writes them)
    if (n > ctx->n && !tail_already_checked) {
        // reference: the Polynomial was truncated at construction (src/polynomial.rs:55-75), so only a
        // non-zero coefficient beyond the SRS makes the degree too high (src/polynomial.rs:201-205)
        uint64_t cnt = n - ctx->n;
        hipLaunchKernelGGL(k_tail_nonzero, dim3((unsigned)((cnt + 255) / 256)), dim3(256), 0, s.stream, d_scalars,
                           (uint64_t)ctx->n, (uint64_t)n, s.small.dev() + 24);
    }
    if (n_msm == 0) {
        s.kind = SLOT_TRIVIAL;
        return KZG_OK;
    }
    int rc = enqueue_msm(ctx, s, d_scalars, is_mont, n_msm, 0, 1, 0, basis);
    if (rc) return rc;
    HIP_TRY(ctx, hipEventRecord(s.done, s.end));
    s.kind = SLOT_COMMIT;
    return KZG_OK;
}

int kzg_commit_submit(kzg_ctx* ctx, int slot, const void* d_coeffs, size_t n) {
    KZG_SINGLE_DEVICE_ONLY(ctx);
    if (!ctx || (!d_coeffs && n)) return KZG_ERR_INVALID_ARG;
    if (n > kMaxCoefficients) return KZG_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(ctx->mu);
    return submit_commit_locked(ctx, slot, (const uint32_t*)d_coeffs, 1, n, false);
}

static int submit_open_locked(kzg_ctx* ctx, int slot, const uint32_t* d_coeffs, size_t n, const uint64_t z[4],
                              const uint64_t y[4], bool owned = false) {
    if (!ctx->n || !ctx->slots_ready) return KZG_ERR_NO_SRS;
    if (slot < 0 || slot >= kNumSlots) return KZG_ERR_INVALID_ARG;
    Slot& s = ctx->slots[slot];
    if (s.kind != (owned ? SLOT_RESERVED : SLOT_IDLE)) return KZG_ERR_BUSY;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    int rc = ensure_poly(ctx, s, n);
    if (rc) return rc;
    s.timing = ctx->timing;
    s.end = s.stream;
    s.job_n = n;
    s.job_batch = 1;
    s.has_quotient = true;
    s.tail_checked = false;
    std::memcpy(s.open_y, y, 32);
    std::memset(&s.times, 0, sizeof s.times);
    if (n == 0) {
        std::memset(s.small.host(), 0, 64 * 4);
        s.kind = SLOT_TRIVIAL;
        return KZG_OK;
    }
    uint32_t zw[8];
    std::memcpy(zw, z, 32);
    if (s.timing) HIP_TRY(ctx, hipEventRecord(s.ev[6], s.stream));
    // small polynomials: one launch for the scan, the flag words and c0; otherwise memset + two launches (c0 written by the first)
    if (!launch_quotient_single(s.stream, d_coeffs, (uint32_t)n, zw, n > 1 ? s.q.dev() : nullptr, s.small.dev())) {
        std::memset(s.small.host(), 0, 64 * 4);
        PolyScratch sc{s.chunk.dev(), s.block.dev(), s.small.dev(), s.small.dev() + 8};
        launch_quotient(s.stream, d_coeffs, (uint32_t)n, zw, n > 1 ? s.q.dev() : nullptr, sc);
    }
    if (s.timing) HIP_TRY(ctx, hipEventRecord(s.ev[7], s.stream));
    size_t nq = n - 1;
    if (nq > ctx->n) {
        // quotient longer than the SRS: too high iff some coefficient with index > srs_len is non-zero
        uint64_t from = ctx->n + 1, cnt = n - from;
        hipLaunchKernelGGL(k_tail_nonzero, dim3((unsigned)((cnt + 255) / 256)), dim3(256), 0, s.stream, d_coeffs, from,
                           (uint64_t)n, s.small.dev() + 24);
        nq = ctx->n;
    }
    if (nq > 0) {
        rc = enqueue_msm(ctx, s, s.q.dev(), 1, nq, 0);
        if (rc) return rc;
    }
    HIP_TRY(ctx, hipEventRecord(s.done, s.end));
    s.kind = nq > 0 ? SLOT_OPEN : SLOT_TRIVIAL;
    return KZG_OK;
}

int kzg_open_submit(kzg_ctx* ctx, int slot, const void* d_coeffs, size_t n, const uint64_t z[4], const uint64_t y[4]) {
    KZG_SINGLE_DEVICE_ONLY(ctx);
    if (!ctx || !z || !y || (!d_coeffs && n)) return KZG_ERR_INVALID_ARG;
    if (n > kMaxCoefficients) return KZG_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(ctx->mu);
    return submit_open_locked(ctx, slot, (const uint32_t*)d_coeffs, n, z, y);
}

// A multiproof on slot `slot`: the scan of P at the k points, the degree check of the quotient (n' - k <= srs_len: no
// non-zero coefficient at index >= srs_len + k), the MSM over q[0 .. n - k).  wait_locked checks the claims first.
static int submit_points_locked(kzg_ctx* ctx, int slot, const uint32_t* d_coeffs, size_t n, const uint64_t* zs,
                                const uint64_t* ys, size_t k, bool owned = false) {
    if (!ctx->n || !ctx->slots_ready) return KZG_ERR_NO_SRS;
    if (slot < 0 || slot >= kNumSlots) return KZG_ERR_INVALID_ARG;
    Slot& s = ctx->slots[slot];
    if (s.kind != (owned ? SLOT_RESERVED : SLOT_IDLE)) return KZG_ERR_BUSY;
    uint64_t ws[4 * KZG_MAX_OPEN_POINTS];
    int rc = points_weights(ctx, zs, k, ws);
    if (rc) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    // (an owned slot's coefficients already sit in its staging buffer, sized by the owner: ensure_poly is a no-op then)
    rc = ensure_poly(ctx, s, n);
    if (rc == KZG_OK) rc = ensure_points(ctx, s, n, k);
    if (rc) return rc;
    s.timing = ctx->timing;
    s.end = s.stream;
    s.job_n = n;
    s.job_batch = 1;
    s.has_quotient = true;
    s.tail_checked = false;
    s.pts_ys.assign((const uint32_t*)ys, (const uint32_t*)ys + 8 * k);
    std::memset(&s.times, 0, sizeof s.times);
    size_t nq = n > k ? n - k : 0;
    if (s.timing) HIP_TRY(ctx, hipEventRecord(s.ev[6], s.stream));
    rc = enqueue_points_scan(ctx, s, d_coeffs, n, zs, ws, k, nq, nq > 0);
    if (rc) return rc;
    if (s.timing) HIP_TRY(ctx, hipEventRecord(s.ev[7], s.stream));
    if (nq > ctx->n) {
        const uint64_t from = ctx->n + k, cnt = n - from;
        hipLaunchKernelGGL(k_tail_nonzero, dim3((unsigned)((cnt + 255) / 256)), dim3(256), 0, s.stream, d_coeffs, from,
                           (uint64_t)n, s.small.dev() + 24);
        nq = ctx->n;
    }
    if (nq > 0) {
        rc = enqueue_msm(ctx, s, s.q.dev(), 1, nq, 0);
        if (rc) return rc;
    }
    s.pts_nq = nq;
    HIP_TRY(ctx, hipEventRecord(s.done, s.end));
    s.kind = SLOT_OPEN_POINTS;
    return KZG_OK;
}

int kzg_open_points_submit(kzg_ctx* ctx, int slot, const void* d_coeffs, size_t n, const uint64_t* zs, const uint64_t* ys,
                           size_t k) {
    KZG_SINGLE_DEVICE_ONLY(ctx);
    if (!ctx || !zs || !ys || (!d_coeffs && n) || n > kMaxCoefficients) return KZG_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(ctx->mu);
    return submit_points_locked(ctx, slot, (const uint32_t*)d_coeffs, n, zs, ys, k);
}

static int wait_locked(kzg_ctx* ctx, int slot, uint64_t out_p1[18]) {
    if (slot < 0 || slot >= kNumSlots) return KZG_ERR_INVALID_ARG;
    Slot& s = ctx->slots[slot];
    if (s.kind == SLOT_IDLE) return KZG_ERR_INVALID_ARG;
    if (s.kind == SLOT_COMMIT_BATCH || s.kind == SLOT_OPEN_BATCH) {
        ctx->last_error = "kzg_wait on a slot that holds a batched job (use kzg_wait_batch / kzg_wait_open_batch)";
        return KZG_ERR_INVALID_ARG;  // the job stays in the slot
    }
    if (s.kind == SLOT_OPEN_COMBINED) {
        ctx->last_error = "kzg_wait on a slot that holds a combined opening (use kzg_wait_combined)";
        return KZG_ERR_INVALID_ARG;  // the job stays in the slot
    }
    if (s.kind == SLOT_OPEN_SETS) {
        ctx->last_error = "kzg_wait on a slot that holds an opening at several point sets (use kzg_wait_sets)";
        return KZG_ERR_INVALID_ARG;  // the job stays in the slot
    }
    if (s.kind == SLOT_RESERVED) return KZG_ERR_BUSY;  // a synchronous call on another thread owns it
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    SlotKind kind = s.kind;
    slot_idle(ctx, s);
    HIP_TRY(ctx, hipEventSynchronize(s.done));
    const bool ran_msm = kind != SLOT_TRIVIAL && !(kind == SLOT_OPEN_POINTS && s.pts_nq == 0);
    if (ran_msm) fill_device_times(s);
    if (s.timing && ran_msm) {
        float ms = 0;
        hipEventElapsedTime(&ms, s.ev[0], s.ev[1]); s.times.digits_ms = ms;
        hipEventElapsedTime(&ms, s.ev[2], s.ev[3]); s.times.scatter_ms = ms;
        fill_accumulate_times(s);
        hipEventElapsedTime(&ms, s.ev[4], s.ev[5]); s.times.reduce_ms = ms;
        if (s.has_quotient) {
            hipEventElapsedTime(&ms, s.ev[6], s.ev[7]); s.times.quotient_ms = ms;
            hipEventElapsedTime(&ms, s.ev[6], s.ev[5]); s.times.total_ms = ms;
        } else {
            hipEventElapsedTime(&ms, s.ev[0], s.ev[5]); s.times.total_ms = ms;
        }
    }
    const uint32_t* hs = s.small.host();
    hf::P1 inf = hf::p1_inf();
    if (kind == SLOT_OPEN_POINTS) {  // every claim first, then the degree (kzg_open's order), then the MSM
        const size_t k = s.pts_ys.size() / 8;
        const uint32_t* vals = points_values(s, k);
        for (size_t i = 0; i < k; i++)
            if (std::memcmp(vals + 8 * i, s.pts_ys.data() + 8 * i, 32) != 0) return KZG_ERR_REMAINDER;
        if (hs[24]) return KZG_ERR_DEGREE_TOO_HIGH;
        write_p1(out_p1, s.pts_nq ? finish_msm(ctx, s) : inf);
        return KZG_OK;
    }
    if (s.has_quotient) {
        // reference order: sub -> divide_by_root (its two errors) -> commit (degree error)
        const size_t n = s.job_n;
        if (n == 0) {  // [] - [y]  (src/polynomial.rs:138-143)
            bool y_zero = true;
            for (int i = 0; i < 8; i++) y_zero &= s.open_y[i] == 0;
            if (!y_zero) return KZG_ERR_CONSTANT_POLY;
            write_p1(out_p1, inf);
            return KZG_OK;
        }
        bool higher_nonzero = hs[0] & 1u;
        if (!higher_nonzero) {  // constant polynomial after truncation (src/polynomial.rs:159-167)
            if (std::memcmp(hs + 16, s.open_y, 32) != 0) return KZG_ERR_CONSTANT_POLY;
            write_p1(out_p1, inf);
            return KZG_OK;
        }
        if (std::memcmp(hs + 8, s.open_y, 32) != 0) return KZG_ERR_REMAINDER;  // P(z) != y
        if (hs[24]) return KZG_ERR_DEGREE_TOO_HIGH;
    } else {
        if (hs[24]) return KZG_ERR_DEGREE_TOO_HIGH;
    }
    if (kind == SLOT_TRIVIAL) {
        write_p1(out_p1, inf);
        return KZG_OK;
    }
    write_p1(out_p1, finish_msm(ctx, s));
    return KZG_OK;
}

int kzg_set_max_batch(kzg_ctx* ctx, size_t max_batch) {
    if (!ctx || max_batch == 0) return KZG_ERR_INVALID_ARG;
    if (ctx->multi) return multi_set_max_batch(ctx->multi, max_batch);  // every device of the context
    std::unique_lock<std::mutex> lk(ctx->mu);
    quiesce(ctx, lk);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    int rc = drain_all(ctx);
    if (rc) return rc;
    for (auto& s : ctx->slots)
        if (s.kind != SLOT_IDLE) return KZG_ERR_BUSY;
    const uint32_t previous = ctx->max_batch;
    ctx->max_batch = (uint32_t)(max_batch > 1024 ? 1024 : max_batch);
    if (!ctx->n) return KZG_OK;  // workspaces are (re)sized when an SRS is resident
    rc = setup_slots(ctx, true);
    if (rc != KZG_OK) {
        // e.g. out of HBM: go back to the size that worked; if even that fails the SRS is dropped (KZG_ERR_NO_SRS next)
        const std::string why = ctx->last_error;
        ctx->max_batch = previous;
        (void)hipGetLastError();
        (void)setup_slots(ctx);
        ctx->last_error = why;
    }
    return rc;
}

size_t kzg_max_batch(const kzg_ctx* ctx) {
    if (ctx && ctx->multi) return kzg_max_batch(multi_kid(ctx->multi, 0));
    return ctx ? ctx->max_batch : 0;
}

static int commit_batch_submit_locked(kzg_ctx* ctx, int slot, const void* d_coeffs, size_t n, size_t batch,
                                      size_t stride_coeffs, bool owned = false, bool lagrange = false) {
    if (!ctx->n || !ctx->slots_ready) return KZG_ERR_NO_SRS;
    MsmBasis basis{};
    if (lagrange && !lagrange_basis(ctx, n, &basis)) return KZG_ERR_NO_SRS;
    if (slot < 0 || slot >= kNumSlots || batch > ctx->max_batch) return KZG_ERR_INVALID_ARG;
    if (n > ctx->n) return KZG_ERR_DEGREE_TOO_HIGH;  // batches take truncated polynomials only
    Slot& s = ctx->slots[slot];
    if (s.kind != (owned ? SLOT_RESERVED : SLOT_IDLE)) return KZG_ERR_BUSY;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    s.timing = ctx->timing;
    s.end = s.stream;
    s.has_quotient = false;
    s.job_n = n;
    s.job_batch = (uint32_t)batch;
    s.tail_checked = true;
    std::memset(&s.times, 0, sizeof s.times);
    std::memset(s.small.host(), 0, 64 * 4);
    int rc = enqueue_msm(ctx, s, (const uint32_t*)d_coeffs, 1, n, 0, (uint32_t)batch, stride_coeffs, lagrange ? &basis : nullptr);
    if (rc) return rc;
    HIP_TRY(ctx, hipEventRecord(s.done, s.end));
    s.kind = SLOT_COMMIT_BATCH;
    return KZG_OK;
}

int kzg_commit_batch_submit(kzg_ctx* ctx, int slot, const void* d_coeffs, size_t n, size_t batch,
                            size_t stride_coeffs) {
    KZG_SINGLE_DEVICE_ONLY(ctx);
    if (!ctx || !d_coeffs || n == 0 || batch == 0 || stride_coeffs < n || n > kMaxCoefficients) return KZG_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(ctx->mu);
    return commit_batch_submit_locked(ctx, slot, d_coeffs, n, batch, stride_coeffs);
}

// out_stride: u64 words between consecutive results (18 = packed)
static int wait_batch_locked(kzg_ctx* ctx, int slot, uint64_t* out_p1s, size_t batch, size_t out_stride = 18) {
    if (slot < 0 || slot >= kNumSlots) return KZG_ERR_INVALID_ARG;
    Slot& s = ctx->slots[slot];
    if (s.kind != SLOT_COMMIT_BATCH || s.job_batch != batch) return KZG_ERR_INVALID_ARG;  // the job stays in the slot
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    slot_idle(ctx, s);
    HIP_TRY(ctx, hipEventSynchronize(s.done));
    fill_device_times(s);
    if (s.timing) {
        float ms = 0;
        (void)hipEventElapsedTime(&ms, s.ev[0], s.ev[1]); s.times.digits_ms = ms;
        (void)hipEventElapsedTime(&ms, s.ev[2], s.ev[3]); s.times.scatter_ms = ms;
        fill_accumulate_times(s);
        (void)hipEventElapsedTime(&ms, s.ev[4], s.ev[5]); s.times.reduce_ms = ms;
        (void)hipEventElapsedTime(&ms, s.ev[0], s.ev[5]); s.times.total_ms = ms;
    }
    // host tails of the batch in parallel (each is ~150 point operations and one inversion)
    const uint32_t B = s.job_batch;
    const uint32_t nthreads = B <= 2 ? 1 : (B < 8 ? B : 8);  // (a thread costs ~50 us to start, a tail ~100)
    auto work = [&](uint32_t t) {
        for (uint32_t p = t; p < B; p += nthreads) write_p1(out_p1s + out_stride * (size_t)p, finish_msm(ctx, s, p, B));
    };
    if (nthreads <= 1) {
        work(0);
    } else {
        std::vector<std::thread> pool;
        for (uint32_t t = 1; t < nthreads; t++) pool.emplace_back(work, t);
        work(0);
        for (auto& th : pool) th.join();
    }
    return KZG_OK;
}

int kzg_wait_batch(kzg_ctx* ctx, int slot, uint64_t* out_p1s, size_t batch) {
    KZG_SINGLE_DEVICE_ONLY(ctx);
    if (!ctx || !out_p1s) return KZG_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(ctx->mu);
    return wait_batch_locked(ctx, slot, out_p1s, batch);
}

// Batched Evaluation::generate_proof: one quotient scan per polynomial (each with its own z, y), then
// ONE batched MSM over the `batch` quotients.
static int open_batch_submit_locked(kzg_ctx* ctx, int slot, const void* d_coeffs, size_t n, size_t batch, size_t stride_coeffs,
                                    const uint64_t* zs, const uint64_t* ys, bool owned = false) {
    if (!ctx->n || !ctx->slots_ready) return KZG_ERR_NO_SRS;
    if (slot < 0 || slot >= kNumSlots || batch > ctx->max_batch) return KZG_ERR_INVALID_ARG;
    if (n - 1 > ctx->n) return KZG_ERR_DEGREE_TOO_HIGH;  // batches take truncated polynomials only
    Slot& s = ctx->slots[slot];
    if (s.kind != (owned ? SLOT_RESERVED : SLOT_IDLE)) return KZG_ERR_BUSY;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    // (an owned slot's coefficients sit in its own staging buffer, which ensure_poly must not reallocate now: the
    // owner sized it before the upload)
    int rc = owned ? KZG_OK : ensure_poly(ctx, s, n * batch);
    if (rc == KZG_OK) rc = s.bsmall.reserve(ctx, batch * 32 * 4, s.stream);
    if (rc) return rc;
    s.timing = ctx->timing;
    s.end = s.stream;
    s.job_n = n;
    s.job_batch = (uint32_t)batch;
    s.has_quotient = true;
    s.tail_checked = true;
    s.open_ys.assign((const uint32_t*)ys, (const uint32_t*)ys + 8 * batch);
    std::memset(&s.times, 0, sizeof s.times);
    std::memset(s.small.host(), 0, 64 * 4);
    std::memset(s.bsmall.host(), 0, batch * 32 * 4);
    if (s.timing) HIP_TRY(ctx, hipEventRecord(s.ev[6], s.stream));
    const size_t nq = n - 1;
    for (size_t p = 0; p < batch; p++) {
        const uint32_t* cp = (const uint32_t*)d_coeffs + p * stride_coeffs * 8;
        uint32_t zw[8];
        std::memcpy(zw, zs + 4 * p, 32);
        uint32_t* sm = s.bsmall.dev() + p * 32;
        PolyScratch sc{s.chunk.dev(), s.block.dev(), sm, sm + 8};  // scratch re-used in stream order
        launch_quotient(s.stream, cp, (uint32_t)n, zw, s.q.dev() + p * nq * 8, sc);
    }
    if (s.timing) HIP_TRY(ctx, hipEventRecord(s.ev[7], s.stream));
    rc = enqueue_msm(ctx, s, s.q.dev(), 1, nq, 0, (uint32_t)batch, nq);
    if (rc) return rc;
    HIP_TRY(ctx, hipEventRecord(s.done, s.end));
    s.kind = SLOT_OPEN_BATCH;
    return KZG_OK;
}

int kzg_open_batch_submit(kzg_ctx* ctx, int slot, const void* d_coeffs, size_t n, size_t batch, size_t stride_coeffs,
                          const uint64_t* zs, const uint64_t* ys) {
    KZG_SINGLE_DEVICE_ONLY(ctx);
    if (!ctx || !d_coeffs || !zs || !ys || n < 2 || batch == 0 || stride_coeffs < n || n > kMaxCoefficients) return KZG_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(ctx->mu);
    return open_batch_submit_locked(ctx, slot, d_coeffs, n, batch, stride_coeffs, zs, ys);
}

static int wait_open_batch_locked(kzg_ctx* ctx, int slot, uint64_t* out_p1s, int* statuses, size_t batch, size_t out_stride = 18,
                                  size_t status_stride = 1) {
    if (slot < 0 || slot >= kNumSlots) return KZG_ERR_INVALID_ARG;
    Slot& s = ctx->slots[slot];
    if (s.kind != SLOT_OPEN_BATCH || s.job_batch != batch || s.open_ys.size() != 8 * batch)
        return KZG_ERR_INVALID_ARG;  // the job stays in the slot
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    slot_idle(ctx, s);
    HIP_TRY(ctx, hipEventSynchronize(s.done));
    fill_device_times(s);
    if (s.timing) {
        float ms = 0;
        (void)hipEventElapsedTime(&ms, s.ev[6], s.ev[7]); s.times.quotient_ms = ms;
        (void)hipEventElapsedTime(&ms, s.ev[0], s.ev[1]); s.times.digits_ms = ms;
        fill_accumulate_times(s);
        (void)hipEventElapsedTime(&ms, s.ev[4], s.ev[5]); s.times.reduce_ms = ms;
        (void)hipEventElapsedTime(&ms, s.ev[6], s.ev[5]); s.times.total_ms = ms;
    }
    const uint32_t B = s.job_batch;
    const hf::P1 inf = hf::p1_inf();
    for (uint32_t p = 0; p < B; p++) {
        const uint32_t* hs = s.bsmall.host() + p * 32;
        const uint32_t* y = s.open_ys.data() + 8 * p;
        uint64_t* out = out_p1s + out_stride * (size_t)p;
        int& status = statuses[status_stride * (size_t)p];
        // reference order: divide_by_root's two errors (src/polynomial.rs:159-167, 184-192)
        if (!(hs[0] & 1u)) {  // constant polynomial after truncation
            if (std::memcmp(hs + 16, y, 32) != 0) status = KZG_ERR_CONSTANT_POLY;
            else { status = KZG_OK; write_p1(out, inf); }
            continue;
        }
        if (std::memcmp(hs + 8, y, 32) != 0) { status = KZG_ERR_REMAINDER; continue; }
        status = KZG_OK;
        write_p1(out, finish_msm(ctx, s, p, B));
    }
    s.open_ys.clear();
    return KZG_OK;
}

int kzg_wait_open_batch(kzg_ctx* ctx, int slot, uint64_t* out_p1s, int* statuses, size_t batch) {
    KZG_SINGLE_DEVICE_ONLY(ctx);
    if (!ctx || !out_p1s || !statuses) return KZG_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(ctx->mu);
    return wait_open_batch_locked(ctx, slot, out_p1s, statuses, batch);
}

int kzg_wait(kzg_ctx* ctx, int slot, uint64_t out_p1[18]) {
    KZG_SINGLE_DEVICE_ONLY(ctx);
    if (!ctx || !out_p1) return KZG_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(ctx->mu);
    return wait_locked(ctx, slot, out_p1);
}

// ---- synchronous host-pointer entry points (what the Rust shim calls) ---------------------------
// The context mutex is held only while a step touches shared state (slot table, enqueue order), never across the
// upload or the wait: the reference's callers are threads of `cargo test` (src/lib.rs:53, 66, 91), and N of them now
// occupy N slots whose jobs pipeline exactly like explicit kzg_*_submit calls.

// waits for the slot's job outside the mutex (kinds that recorded `done`), then collects it
static void await_unlocked(std::unique_lock<std::mutex>& lk, Slot& s) {
    if (s.kind == SLOT_TRIVIAL || s.kind == SLOT_RESERVED || s.kind == SLOT_IDLE) return;
    lk.unlock();
    (void)hipEventSynchronize(s.done);
    lk.lock();
}

struct HostTrace {  // phase stopwatch of one synchronous call
    kzg_ctx* ctx;
    std::chrono::steady_clock::time_point t;
    explicit HostTrace(kzg_ctx* c) : ctx(c) { if (c->host_trace) t = std::chrono::steady_clock::now(); }
    void mark(int phase) {
        if (!ctx->host_trace) return;
        const auto now = std::chrono::steady_clock::now();
        ctx->trace_ns[phase] += (uint64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(now - t).count();
        t = now;
    }
};

static int commit_host(kzg_ctx* ctx, const void* scalars, int is_mont, size_t n, uint64_t out_p1[18]) {
    if (!ctx || !out_p1 || (!scalars && n)) return KZG_ERR_INVALID_ARG;
    if (n > kMaxCoefficients) return KZG_ERR_INVALID_ARG;
    if (ctx->multi) return multi_commit(ctx->multi, scalars, is_mont, n, out_p1);
    HostTrace tr(ctx);
    std::unique_lock<std::mutex> lk(ctx->mu);
    if (!ctx->n || !ctx->slots_ready) return KZG_ERR_NO_SRS;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (n > ctx->n && host_tail_nonzero((const uint64_t*)scalars, ctx->n, n)) return KZG_ERR_DEGREE_TOO_HIGH;
    const int slot = reserve_slot(ctx, lk, true);
    if (slot < 0) return KZG_ERR_BUSY;
    Slot& s = ctx->slots[slot];
    const size_t n_dev = n < ctx->n ? n : ctx->n;
    int rc = ensure_poly(ctx, s, n_dev);
    tr.mark(0);
    if (rc == KZG_OK) rc = upload_unlocked(ctx, lk, s, s.stage.dev(), scalars, n_dev * 32);
    tr.mark(1);
    if (rc == KZG_OK) rc = submit_commit_locked(ctx, slot, s.stage.dev(), is_mont, n_dev, true, true);
    tr.mark(2);
    if (rc == KZG_OK) {
        await_unlocked(lk, s);
        tr.mark(3);
        rc = wait_locked(ctx, slot, out_p1);
        tr.mark(4);
    }
    release_owned(ctx, slot);
    ctx->trace_calls++;
    return rc;
}

int kzg_commit(kzg_ctx* ctx, const uint64_t* coeffs, size_t n, uint64_t out_p1[18]) {
    return commit_host(ctx, coeffs, 1, n, out_p1);
}
int kzg_commit_le_bytes(kzg_ctx* ctx, const uint8_t* scalars_le, size_t n, uint64_t out_p1[18]) {
    return commit_host(ctx, scalars_le, 0, n, out_p1);
}

int kzg_open(kzg_ctx* ctx, const uint64_t* coeffs, size_t n, const uint64_t z[4], const uint64_t y[4],
             uint64_t out_p1[18]) {
    if (!ctx || !out_p1 || !z || !y || (!coeffs && n)) return KZG_ERR_INVALID_ARG;
    if (n > kMaxCoefficients) return KZG_ERR_INVALID_ARG;
    if (ctx->multi) return multi_open(ctx->multi, coeffs, n, z, y, out_p1);
    std::unique_lock<std::mutex> lk(ctx->mu);
    if (!ctx->n || !ctx->slots_ready) return KZG_ERR_NO_SRS;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const int slot = reserve_slot(ctx, lk, true);
    if (slot < 0) return KZG_ERR_BUSY;
    Slot& s = ctx->slots[slot];
    int rc = ensure_poly(ctx, s, n);
    if (rc == KZG_OK) rc = upload_unlocked(ctx, lk, s, s.stage.dev(), coeffs, n * 32);
    if (rc == KZG_OK) rc = submit_open_locked(ctx, slot, s.stage.dev(), n, z, y, true);
    if (rc == KZG_OK) {
        await_unlocked(lk, s);
        rc = wait_locked(ctx, slot, out_p1);
    }
    release_owned(ctx, slot);
    return rc;
}

int kzg_open_points(kzg_ctx* ctx, const uint64_t* coeffs, size_t n, const uint64_t* zs, const uint64_t* ys, size_t k,
                    uint64_t out_p1[18]) {
    if (!ctx || !out_p1 || !zs || !ys || (!coeffs && n) || n > kMaxCoefficients) return KZG_ERR_INVALID_ARG;
    if (k < 1 || k > KZG_MAX_OPEN_POINTS) return KZG_ERR_INVALID_ARG;
    if (ctx->multi) return multi_open_points(ctx->multi, coeffs, n, zs, ys, k, out_p1);
    std::unique_lock<std::mutex> lk(ctx->mu);
    if (!ctx->n || !ctx->slots_ready) return KZG_ERR_NO_SRS;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const int slot = reserve_slot(ctx, lk, true);
    if (slot < 0) return KZG_ERR_BUSY;
    Slot& s = ctx->slots[slot];
    int rc = ensure_poly(ctx, s, n);
    if (rc == KZG_OK) rc = upload_unlocked(ctx, lk, s, s.stage.dev(), coeffs, n * 32);
    if (rc == KZG_OK) rc = submit_points_locked(ctx, slot, s.stage.dev(), n, zs, ys, k, true);
    if (rc == KZG_OK) {
        await_unlocked(lk, s);
        rc = wait_locked(ctx, slot, out_p1);
    }
    release_owned(ctx, slot);
    return rc;
}

// ---- combined openings: t polynomials, one point, one proof ---------------------------------
namespace {
// the slot's buffers for passes of at most t_pass polynomials of n coefficients; stage_coeffs: room in cin (host-pointer
// passes), 0 when the polynomials are resident (slot basics already there)
int ensure_combined(kzg_ctx* ctx, Slot& s, size_t n, size_t t_pass, size_t stage_coeffs) {
    int rc = s.ctab.reserve(ctx, kCombineTabLen * sizeof(Fr30));
    if (rc == KZG_OK) rc = s.cvals.reserve(ctx, kCombineMax * 32);
    if (rc) return rc;
    for (auto& e : s.cmb_ev)
        if (!e) HIP_TRY(ctx, hipEventCreate(&e));
    rc = s.cpart.reserve(ctx, t_pass * combine_tiles((uint32_t)(n ? n : 1)) * kCombinePartialWords * 4, s.stream);
    if (rc == KZG_OK) rc = s.cin.reserve(ctx, stage_coeffs * 32, s.stream);
    return rc;
}
// every multiplier of one call: the 16 + 16 tables and the stride of z (a lane's power inside a tile) and of W = z^2048
// (a tile's power inside the polynomial), then gamma^i -- 66 + t host products -- copied to the slot's table on the front stream
void combine_fill_powers(Fr30* tab, const hf::Fr& z) {  // entries [0, kCombineTabGamma)
    auto fill = [&](const hf::Fr& x, uint32_t at_a, uint32_t at_b, uint32_t at_256) {
        const hf::Fr x16 = hf::fr_pow(x, 16);
        hf::Fr a = hf::kFrOne, b = hf::kFrOne;
        for (int e = 0; e < 16; e++) {
            tab[at_a + e] = fr30_arg_from_mont256(a);
            tab[at_b + e] = fr30_arg_from_mont256(b);
            a = hf::fr_mul(a, x16);
            b = hf::fr_mul(b, x);
        }
        tab[at_256] = fr30_arg_from_mont256(a);  // (x^16)^16
        return a;
    };
    const hf::Fr z256 = fill(z, kCombineTabPa, kCombineTabPb, kCombineTabZ256);
    fill(hf::fr_pow(z256, kCombineTile / 256), kCombineTabWa, kCombineTabWb, kCombineTabW256);
}
int combined_upload_table(kzg_ctx* ctx, Slot& s, const hf::Fr& z, const hf::Fr& gamma, size_t t) {
    Fr30* tab = (Fr30*)s.ctab.h;
    combine_fill_powers(tab, z);
    hf::Fr g = hf::kFrOne;
    for (size_t i = 0; i < t; i++) {
        tab[kCombineTabGamma + i] = fr30_arg_from_mont256(g);
        g = hf::fr_mul(g, gamma);
    }
    HIP_TRY(ctx, hipMemcpyAsync(s.ctab.d, s.ctab.h, (kCombineTabGamma + t) * sizeof(Fr30), hipMemcpyHostToDevice, s.stream));
    return KZG_OK;
}
// one pass on the front stream: polynomials first .. first + cnt (device memory) into F (s.stage, carried from the earlier
// passes when first > 0) and their values into the slot's value words
int combined_pass(kzg_ctx* ctx, Slot& s, const uint32_t* d_coeffs, size_t n, size_t cnt, size_t stride, size_t first) {
    if (s.timing) HIP_TRY(ctx, hipEventRecord(s.cmb_ev[0], s.stream));
    launch_combine_eval(s.stream, d_coeffs, (uint32_t)n, (uint32_t)cnt, stride, (const Fr30*)s.ctab.d, (uint32_t)first, first > 0,
                        s.stage.dev(), s.cpart.dev(), s.cvals.dev() + 8 * first);
    if (s.timing) HIP_TRY(ctx, hipEventRecord(s.cmb_ev[1], s.stream));
    HIP_TRY(ctx, hipGetLastError());
    return KZG_OK;
}
bool fr_arg_below_r(const uint64_t v[4], hf::Fr* out) {
    std::memcpy(out->l, v, 32);
    return !hf::fr_geq(*out, hf::kFrMod);
}
// the arguments every combined call shares; z, gamma may be null where the call takes none
int combined_check(kzg_ctx* ctx, const char* what, const void* coeffs, size_t n, size_t t, size_t stride, const uint64_t* z,
                   const uint64_t* gamma, hf::Fr* zf, hf::Fr* gf) {
    auto invalid = [&](const char* why) {
        ctx->last_error = std::string(what) + ": " + why;
        return KZG_ERR_INVALID_ARG;
    };
    if (t < 1 || t > KZG_MAX_COMBINE) return invalid("t must be in [1, KZG_MAX_COMBINE]");
    if (!coeffs && n) return invalid("null coefficients");
    if (n > kMaxCoefficients) return invalid("too many coefficients");
    if (t > 1 && stride < n) return invalid("stride below n");
    *zf = hf::Fr{{0, 0, 0, 0}};
    *gf = hf::Fr{{0, 0, 0, 0}};
    if (z && !fr_arg_below_r(z, zf)) return invalid("the point z is not below r");
    if (gamma && !fr_arg_below_r(gamma, gf)) return invalid("gamma is not below r");
    return KZG_OK;
}
// host polynomials [first, first + cnt) -> the slot's pass buffer, n coefficients each, back to back; without the mutex
int combined_stage_unlocked(kzg_ctx* ctx, std::unique_lock<std::mutex>& lk, Slot& s, const uint64_t* coeffs, size_t n, size_t stride,
                            size_t first, size_t cnt) {
    if (stride == n || cnt == 1)
        return copy_unlocked(ctx, lk, s.stream, s.cin.dev(), coeffs + 4 * first * stride, cnt * n * 32, hipMemcpyHostToDevice, kCopyCoeffs);
    int rc = KZG_OK;
    for (size_t i = 0; i < cnt && rc == KZG_OK; i++)
        rc = copy_unlocked(ctx, lk, s.stream, s.cin.dev() + 8 * i * n, coeffs + 4 * (first + i) * stride, n * 32, hipMemcpyHostToDevice,
                           kCopyCoeffs);
    return rc;
}
// all passes of a host-pointer call: at most max_batch polynomials per launch
int combined_host_passes(kzg_ctx* ctx, std::unique_lock<std::mutex>& lk, Slot& s, const uint64_t* coeffs, size_t n, size_t t,
                         size_t stride, const hf::Fr& z, const hf::Fr& gamma) {
    const size_t group = std::min<size_t>(t, ctx->max_batch ? ctx->max_batch : 1);
    int rc = ensure_poly(ctx, s, n);
    if (rc == KZG_OK) rc = ensure_combined(ctx, s, n, group, group * n);
    if (rc == KZG_OK) rc = combined_upload_table(ctx, s, z, gamma, t);
    for (size_t first = 0; first < t && rc == KZG_OK; first += group) {
        const size_t cnt = std::min(group, t - first);
        rc = combined_stage_unlocked(ctx, lk, s, coeffs, n, stride, first, cnt);
        if (rc == KZG_OK) rc = combined_pass(ctx, s, s.cin.dev(), n, cnt, n, first);
    }
    return rc;
}
// the opening of F (n coefficients in s.stage) at z behind the passes, as submit_open_locked runs it on a caller's buffer;
// the prover has no claim, so F(z) is only computed, not compared
int combined_enqueue_open(kzg_ctx* ctx, Slot& s, size_t n, size_t t, const uint64_t z[4]) {
    s.job_n = n;
    s.job_batch = 1;
    s.has_quotient = true;
    s.tail_checked = false;
    s.cmb_t = t;
    s.pts_nq = 0;
    std::memset(s.small.host(), 0, 64 * 4);  // (nothing in flight writes them: the passes do not touch the flag words)
    if (n > 0) {
        uint32_t zw[8];
        std::memcpy(zw, z, 32);
        if (s.timing) HIP_TRY(ctx, hipEventRecord(s.ev[6], s.stream));
        if (!launch_quotient_single(s.stream, s.stage.dev(), (uint32_t)n, zw, n > 1 ? s.q.dev() : nullptr, s.small.dev())) {
            PolyScratch sc{s.chunk.dev(), s.block.dev(), s.small.dev(), s.small.dev() + 8};
            launch_quotient(s.stream, s.stage.dev(), (uint32_t)n, zw, n > 1 ? s.q.dev() : nullptr, sc);
        }
        if (s.timing) HIP_TRY(ctx, hipEventRecord(s.ev[7], s.stream));
        size_t nq = n - 1;
        if (nq > ctx->n) {  // too high iff some coefficient of F with index > srs_len is non-zero
            const uint64_t from = ctx->n + 1, cnt = n - from;
            hipLaunchKernelGGL(k_tail_nonzero, dim3((unsigned)((cnt + 255) / 256)), dim3(256), 0, s.stream, s.stage.dev(), from,
                               (uint64_t)n, s.small.dev() + 24);
            nq = ctx->n;
        }
        if (nq > 0) {
            int rc = enqueue_msm(ctx, s, s.q.dev(), 1, nq, 0);
            if (rc) return rc;
        }
        s.pts_nq = nq;
    }
    HIP_TRY(ctx, hipEventRecord(s.done, s.end));
    s.kind = SLOT_OPEN_COMBINED;
    return KZG_OK;
}
int combined_job_start(kzg_ctx* ctx, Slot& s, size_t t) {
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    s.timing = ctx->timing;
    s.end = s.stream;
    s.combine_ms = 0;
    std::memset(&s.times, 0, sizeof s.times);
    int rc = ensure_combined(ctx, s, 0, 0, 0);
    if (rc == KZG_OK) std::memset(s.cvals.host(), 0, 32 * t);  // (the slot holds no job in flight)
    return rc;
}

int wait_combined_locked(kzg_ctx* ctx, int slot, uint64_t* out_ys, uint64_t out_p1[18]) {
    if (slot < 0 || slot >= kNumSlots) return KZG_ERR_INVALID_ARG;
    Slot& s = ctx->slots[slot];
    if (s.kind == SLOT_RESERVED) return KZG_ERR_BUSY;  // a synchronous call on another thread owns it
    if (s.kind != SLOT_OPEN_COMBINED) {
        if (s.kind != SLOT_IDLE) ctx->last_error = "kzg_wait_combined on a slot that holds another kind of job";
        return KZG_ERR_INVALID_ARG;  // the job stays in the slot
    }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    slot_idle(ctx, s);
    HIP_TRY(ctx, hipEventSynchronize(s.done));
    const bool ran_msm = s.pts_nq > 0;
    if (ran_msm) fill_device_times(s);
    if (s.timing && s.job_n > 0) {
        float ms = 0;
        if (hipEventElapsedTime(&ms, s.cmb_ev[0], s.cmb_ev[1]) == hipSuccess) s.combine_ms = ms;
        if (ran_msm) {
            hipEventElapsedTime(&ms, s.ev[0], s.ev[1]); s.times.digits_ms = ms;
            hipEventElapsedTime(&ms, s.ev[2], s.ev[3]); s.times.scatter_ms = ms;
            fill_accumulate_times(s);
            hipEventElapsedTime(&ms, s.ev[4], s.ev[5]); s.times.reduce_ms = ms;
            hipEventElapsedTime(&ms, s.ev[6], s.ev[7]); s.times.quotient_ms = ms;
            hipEventElapsedTime(&ms, s.ev[6], s.ev[5]); s.times.total_ms = ms;
        }
    }
    std::memcpy(out_ys, s.cvals.host(), 32 * s.cmb_t);
    const uint32_t* hs = s.small.host();
    // F after the reference's truncation: no non-zero coefficient above the constant one -> infinity, like kzg_open_points
    if (s.job_n == 0 || !(hs[0] & 1u)) {
        write_p1(out_p1, hf::p1_inf());
        return KZG_OK;
    }
    if (hs[24]) return KZG_ERR_DEGREE_TOO_HIGH;
    write_p1(out_p1, ran_msm ? finish_msm(ctx, s) : hf::p1_inf());
    return KZG_OK;
}

// the two hooks: every pass of the host-pointer call without the opening (no SRS needed)
int combined_hook(kzg_ctx* ctx, const char* what, const uint64_t* coeffs, size_t n, size_t t, size_t stride, const uint64_t* z,
                  const uint64_t* gamma, uint64_t* out_f, uint64_t* out_ys) {
    hf::Fr zf, gf;
    std::unique_lock<std::mutex> lk(ctx->mu);
    int rc = combined_check(ctx, what, coeffs, n, t, stride, z, gamma, &zf, &gf);
    if (rc) return rc;
    if (out_ys) std::memset(out_ys, 0, 32 * t);
    if (n == 0) return KZG_OK;
    const int slot = reserve_slot(ctx, lk, true);
    if (slot < 0) return KZG_ERR_BUSY;
    SlotLease lease{ctx, slot};
    Slot& s = ctx->slots[slot];
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    rc = ensure_slot_basics(ctx, s);
    if (rc == KZG_OK) rc = combined_job_start(ctx, s, t);
    if (rc == KZG_OK) rc = combined_host_passes(ctx, lk, s, coeffs, n, t, stride, zf, gf);
    if (rc) return rc;
    HIP_TRY(ctx, hipStreamSynchronize(s.stream));
    if (out_ys) std::memcpy(out_ys, s.cvals.host(), 32 * t);
    if (out_f) HIP_TRY(ctx, hipMemcpy(out_f, s.stage.dev(), n * 32, hipMemcpyDeviceToHost));
    return KZG_OK;
}
}  // namespace

int kzg_open_combined(kzg_ctx* ctx, const uint64_t* coeffs, size_t n, size_t t, size_t stride, const uint64_t z[4],
                      const uint64_t gamma[4], uint64_t* out_ys, uint64_t out_p1[18]) {
    if (!ctx || !z || !gamma || !out_ys || !out_p1) return KZG_ERR_INVALID_ARG;
    hf::Fr zf, gf;
    std::unique_lock<std::mutex> lk(ctx->mu);
    int rc = combined_check(ctx, "kzg_open_combined", coeffs, n, t, stride, z, gamma, &zf, &gf);
    if (rc) return rc;
    if (ctx->multi) {
        ctx->last_error.clear();  // (kzg_last_error then reads the devices' side)
        lk.unlock();
        return multi_open_combined(ctx->multi, coeffs, n, t, stride, z, gamma, out_ys, out_p1);
    }
    if (!ctx->n || !ctx->slots_ready) return KZG_ERR_NO_SRS;
    const int slot = reserve_slot(ctx, lk, true);
    if (slot < 0) return KZG_ERR_BUSY;
    Slot& s = ctx->slots[slot];
    rc = combined_job_start(ctx, s, t);
    if (rc == KZG_OK && n) rc = combined_host_passes(ctx, lk, s, coeffs, n, t, stride, zf, gf);
    if (rc == KZG_OK) rc = combined_enqueue_open(ctx, s, n, t, z);
    if (rc == KZG_OK) {
        await_unlocked(lk, s);
        rc = wait_combined_locked(ctx, slot, out_ys, out_p1);
    }
    release_owned(ctx, slot);
    return rc;
}

int kzg_open_combined_submit(kzg_ctx* ctx, int slot, const void* d_coeffs, size_t n, size_t t, size_t stride, const uint64_t z[4],
                             const uint64_t gamma[4]) {
    KZG_SINGLE_DEVICE_ONLY(ctx);
    if (!ctx || !z || !gamma) return KZG_ERR_INVALID_ARG;
    hf::Fr zf, gf;
    std::lock_guard<std::mutex> lk(ctx->mu);
    int rc = combined_check(ctx, "kzg_open_combined_submit", d_coeffs, n, t, stride, z, gamma, &zf, &gf);
    if (rc) return rc;
    if (!ctx->n || !ctx->slots_ready) return KZG_ERR_NO_SRS;
    if (slot < 0 || slot >= kNumSlots) return KZG_ERR_INVALID_ARG;
    Slot& s = ctx->slots[slot];
    if (s.kind != SLOT_IDLE) return KZG_ERR_BUSY;
    rc = combined_job_start(ctx, s, t);
    if (rc == KZG_OK && n) {  // all t polynomials in one launch
        rc = ensure_poly(ctx, s, n);
        if (rc == KZG_OK) rc = ensure_combined(ctx, s, n, t, 0);
        if (rc == KZG_OK) rc = combined_upload_table(ctx, s, zf, gf, t);
        if (rc == KZG_OK) rc = combined_pass(ctx, s, (const uint32_t*)d_coeffs, n, t, stride, 0);
    }
    if (rc == KZG_OK) rc = combined_enqueue_open(ctx, s, n, t, z);
    return rc;
}

int kzg_wait_combined(kzg_ctx* ctx, int slot, uint64_t* out_ys, uint64_t out_p1[18]) {
    KZG_SINGLE_DEVICE_ONLY(ctx);
    if (!ctx || !out_ys || !out_p1) return KZG_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(ctx->mu);
    return wait_combined_locked(ctx, slot, out_ys, out_p1);
}

int kzg_get_combine_ms(kzg_ctx* ctx, int slot, float* out_ms) {
    if (!ctx || ctx->multi || !out_ms || slot < 0 || slot >= kNumSlots) return KZG_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(ctx->mu);
    *out_ms = ctx->slots[slot].combine_ms;
    return KZG_OK;
}

int kzg_combine_polys(kzg_ctx* ctx, const uint64_t* coeffs, size_t n, size_t t, size_t stride, const uint64_t gamma[4],
                      uint64_t* out_f) {
    if (!ctx || !gamma || (!out_f && n)) return KZG_ERR_INVALID_ARG;
    if (ctx->multi) return kzg_combine_polys(multi_kid(ctx->multi, 0), coeffs, n, t, stride, gamma, out_f);  // needs no SRS
    return combined_hook(ctx, "kzg_combine_polys", coeffs, n, t, stride, nullptr, gamma, out_f, nullptr);
}

int kzg_evaluate_batch_at(kzg_ctx* ctx, const uint64_t* coeffs, size_t n, size_t t, size_t stride, const uint64_t z[4],
                          uint64_t* out_ys) {
    if (!ctx || !z || !out_ys) return KZG_ERR_INVALID_ARG;
    if (ctx->multi) return kzg_evaluate_batch_at(multi_kid(ctx->multi, 0), coeffs, n, t, stride, z, out_ys);  // needs no SRS
    return combined_hook(ctx, "kzg_evaluate_batch_at", coeffs, n, t, stride, z, nullptr, nullptr, out_ys);
}

// ---- openings at several point sets: polynomial i on set set_of[i], one proof ----------------------
namespace {
constexpr uint32_t kSetsMultBase = kSetsMaxPoints * kCombineTabGamma;  // the pass tables: 66 powers per point, then the multipliers
constexpr uint32_t kSetsTabLen = kSetsMultBase + kSetsMaxValues;
static_assert(KZG_MAX_SETS == kSetsMax && KZG_MAX_SET_POINTS == kSetsMaxPoints, "header and engine disagree");
static_assert(KZG_MAX_SET_POINTS <= KZG_MAX_OPEN_POINTS, "the scans use the multiproof's root buffers");

// what the arrays of a call say, checked: the distinct points T, every set's weights, and per point of T the list of
// polynomials opened there with their multipliers gamma^i w_(g(i),p)
struct SetsPlan {
    size_t t = 0, m = 0, npts = 0, nvals = 0, min_len = 0, max_len = 0;
    hf::Fr gamma;
    hf::Fr pts[KZG_MAX_SET_POINTS];                 // T, in order of first appearance
    uint32_t set_first[KZG_MAX_SETS] = {};          // first entry of set g in zs
    uint32_t set_len[KZG_MAX_SETS] = {};
    uint8_t pt_of[KZG_MAX_SETS][KZG_MAX_SET_POINTS];  // index in T of point j of set g
    int8_t pos[KZG_MAX_SETS][KZG_MAX_SET_POINTS];     // position of point r of T in set g, or -1
    hf::Fr w[KZG_MAX_SETS][KZG_MAX_SET_POINTS];       // w_(g,p) by position in the set
    uint32_t off[KZG_MAX_SET_POINTS + 1] = {};      // the list of point r: sel[off[r] .. off[r + 1])
    std::vector<uint32_t> set_of;                   // t
    std::vector<uint32_t> val_first;                // first entry of polynomial i in out_ys
    std::vector<uint32_t> sel;                      // polynomials opened at point r, increasing
    std::vector<hf::Fr> mult;                       // gamma^i w_(g(i),p), parallel to sel
    std::vector<uint32_t> vmap;                     // entry e of out_ys sits at pass-order index vmap[e]
};
// t, m and the pointers are the caller's business; everything else about the sets is refused here, in the header's order
bool sets_plan(SetsPlan& P, std::string& why, size_t t, const uint32_t* set_of, const uint32_t* set_len, size_t m,
               const uint64_t* zs, const uint64_t* gamma) {
    P.t = t;
    P.m = m;
    uint32_t at = 0;
    for (size_t g = 0; g < m; g++) {
        if (set_len[g] == 0) return why = "an empty point set", false;
        if (set_len[g] > KZG_MAX_SET_POINTS) return why = "a set of more than KZG_MAX_SET_POINTS points", false;
        P.set_first[g] = at;
        P.set_len[g] = set_len[g];
        at += set_len[g];
    }
    bool used[KZG_MAX_SETS] = {};
    P.set_of.assign(set_of, set_of + t);
    for (size_t i = 0; i < t; i++) {
        if (set_of[i] >= m) return why = "set_of names a set that does not exist", false;
        used[set_of[i]] = true;
    }
    for (size_t g = 0; g < m; g++)
        if (!used[g]) return why = "a point set no polynomial is opened on", false;
    P.npts = 0;
    std::memset(P.pos, -1, sizeof P.pos);
    P.min_len = KZG_MAX_SET_POINTS;
    P.max_len = 0;
    for (size_t g = 0; g < m; g++) {
        hf::Fr z[KZG_MAX_SET_POINTS];
        const size_t k = P.set_len[g];
        for (size_t j = 0; j < k; j++)
            if (!fr_arg_below_r(zs + 4 * (P.set_first[g] + j), &z[j])) return why = "a point is not below r", false;
        if (!hf::fr_point_weights(z, k, P.w[g])) return why = "two equal points within one set", false;
        for (size_t j = 0; j < k; j++) {
            size_t r = 0;
            while (r < P.npts && std::memcmp(P.pts[r].l, z[j].l, 32) != 0) r++;
            if (r == P.npts) {
                if (P.npts == KZG_MAX_SET_POINTS) return why = "more than KZG_MAX_SET_POINTS distinct points", false;
                P.pts[P.npts++] = z[j];
            }
            P.pt_of[g][j] = (uint8_t)r;
            P.pos[g][r] = (int8_t)j;
        }
        P.min_len = std::min(P.min_len, k);
        P.max_len = std::max(P.max_len, k);
    }
    if (!fr_arg_below_r(gamma, &P.gamma)) return why = "gamma is not below r", false;
    P.val_first.resize(t);
    P.nvals = 0;
    for (size_t i = 0; i < t; i++) {
        P.val_first[i] = (uint32_t)P.nvals;
        P.nvals += P.set_len[set_of[i]];
    }
    std::vector<hf::Fr> gpow(t);
    hf::Fr gp = hf::kFrOne;
    for (size_t i = 0; i < t; i++) {
        gpow[i] = gp;
        gp = hf::fr_mul(gp, P.gamma);
    }
    P.sel.clear();
    P.mult.clear();
    P.vmap.assign(P.nvals, 0);
    for (size_t r = 0; r < P.npts; r++) {
        P.off[r] = (uint32_t)P.sel.size();
        for (size_t i = 0; i < t; i++) {
            const uint32_t g = set_of[i];
            const int j = P.pos[g][r];
            if (j < 0) continue;
            P.vmap[P.val_first[i] + j] = (uint32_t)P.sel.size();
            P.sel.push_back((uint32_t)i);
            P.mult.push_back(hf::fr_mul(gpow[i], P.w[g][j]));
        }
    }
    P.off[P.npts] = (uint32_t)P.sel.size();
    return true;
}
// the arguments every prover call shares
int sets_check(kzg_ctx* ctx, const char* what, const void* coeffs, size_t n, size_t t, size_t stride, const uint32_t* set_of,
               const uint32_t* set_len, size_t m, const uint64_t* zs, const uint64_t* gamma, SetsPlan& plan) {
    auto invalid = [&](const std::string& why) {
        ctx->last_error = std::string(what) + ": " + why;
        return KZG_ERR_INVALID_ARG;
    };
    if (t < 1 || t > KZG_MAX_COMBINE) return invalid("t must be in [1, KZG_MAX_COMBINE]");
    if (m < 1 || m > KZG_MAX_SETS) return invalid("m must be in [1, KZG_MAX_SETS]");
    std::string why;
    if (!sets_plan(plan, why, t, set_of, set_len, m, zs, gamma)) return invalid(why);
    if (!coeffs && n) return invalid("null coefficients");
    if (n > kMaxCoefficients) return invalid("too many coefficients");
    if (t > 1 && stride < n) return invalid("stride below n");
    return KZG_OK;
}

// the slot's buffers for |T| = npts points over n coefficients (slot basics already there)
int ensure_sets(kzg_ctx* ctx, Slot& s, size_t n, size_t npts) {
    int rc = s.stab.reserve(ctx, kSetsTabLen * sizeof(Fr30));
    if (rc == KZG_OK) rc = s.ssel.reserve(ctx, kSetsMaxValues * 4);
    if (rc == KZG_OK) rc = s.svals.reserve(ctx, kSetsMaxValues * 32);
    if (rc == KZG_OK) rc = s.sg.reserve(ctx, npts * n * 32, s.stream);
    return rc;
}
int sets_job_start(kzg_ctx* ctx, Slot& s, const SetsPlan& plan) {
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    s.timing = ctx->timing;
    s.end = s.stream;
    s.combine_ms = 0;
    std::memset(&s.times, 0, sizeof s.times);
    int rc = ensure_combined(ctx, s, 0, 0, 0);
    if (rc == KZG_OK) rc = ensure_sets(ctx, s, 0, 0);
    if (rc == KZG_OK) std::memset(s.svals.host(), 0, 32 * plan.nvals);  // (the slot holds no job in flight)
    return rc;
}
// every buffer of a job whose passes take at most t_pass polynomials; stage_coeffs as in ensure_combined
int sets_ensure_all(kzg_ctx* ctx, Slot& s, const SetsPlan& plan, size_t n, size_t t_pass, size_t stage_coeffs) {
    int rc = ensure_poly(ctx, s, n);
    if (rc == KZG_OK) rc = ensure_points(ctx, s, n, plan.npts);
    if (rc == KZG_OK) rc = ensure_combined(ctx, s, n, t_pass, stage_coeffs);
    if (rc == KZG_OK) rc = ensure_sets(ctx, s, n, plan.npts);
    return rc;
}
// the multipliers of one call -- 66 host products per distinct point, the multipliers and the lists as planned -- copied to
// the slot's tables on the front stream
int sets_upload_tables(kzg_ctx* ctx, Slot& s, const SetsPlan& plan) {
    Fr30* tab = (Fr30*)s.stab.h;
    for (size_t r = 0; r < plan.npts; r++) combine_fill_powers(tab + r * kCombineTabGamma, plan.pts[r]);
    for (size_t e = 0; e < plan.sel.size(); e++) {
        tab[kSetsMultBase + e] = fr30_arg_from_mont256(plan.mult[e]);
        s.ssel.host()[e] = plan.sel[e];
    }
    HIP_TRY(ctx, hipMemcpyAsync(s.stab.d, s.stab.h, (kSetsMultBase + plan.sel.size()) * sizeof(Fr30), hipMemcpyHostToDevice, s.stream));
    HIP_TRY(ctx, hipMemcpyAsync(s.ssel.dev(), s.ssel.host(), plan.sel.size() * 4, hipMemcpyHostToDevice, s.stream));
    return KZG_OK;
}
// The passes over polynomials first .. first + cnt (device memory, polynomial `first` at d_coeffs): one per distinct point
// that one of them is opened at.  A point's list is sorted, so these polynomials are a run [j0, j1) of it; written[r] says
// whether G_r holds the sum of earlier calls (carried) or nothing yet.
int sets_passes(kzg_ctx* ctx, Slot& s, const SetsPlan& plan, const uint32_t* d_coeffs, size_t n, size_t stride, size_t first,
                size_t cnt, bool* written) {
    if (s.timing) HIP_TRY(ctx, hipEventRecord(s.cmb_ev[0], s.stream));
    for (size_t r = 0; r < plan.npts; r++) {
        const auto lo = plan.sel.begin() + plan.off[r], hi = plan.sel.begin() + plan.off[r + 1];
        const size_t j0 = std::lower_bound(lo, hi, (uint32_t)first) - plan.sel.begin();
        const size_t j1 = std::lower_bound(lo, hi, (uint32_t)(first + cnt)) - plan.sel.begin();
        if (j0 == j1) continue;
        launch_sets_combine(s.stream, d_coeffs, (uint32_t)n, (uint32_t)(j1 - j0), stride, (const Fr30*)s.stab.d + r * kCombineTabGamma,
                            (const Fr30*)s.stab.d + kSetsMultBase + j0, s.ssel.dev() + j0, (uint32_t)first, written[r],
                            s.sg.dev() + 8 * r * n, s.cpart.dev(), s.svals.dev() + 8 * j0);
        written[r] = true;
    }
    if (s.timing) HIP_TRY(ctx, hipEventRecord(s.cmb_ev[1], s.stream));
    HIP_TRY(ctx, hipGetLastError());
    return KZG_OK;
}
// all passes of a host-pointer call: at most max_batch polynomials are resident at a time, every G_p is carried
int sets_host_passes(kzg_ctx* ctx, std::unique_lock<std::mutex>& lk, Slot& s, const SetsPlan& plan, const uint64_t* coeffs, size_t n,
                     size_t stride) {
    const size_t t = plan.t, group = std::min<size_t>(t, ctx->max_batch ? ctx->max_batch : 1);
    int rc = sets_ensure_all(ctx, s, plan, n, group, group * n);
    if (rc == KZG_OK) rc = sets_upload_tables(ctx, s, plan);
    bool written[KZG_MAX_SET_POINTS] = {};
    for (size_t first = 0; first < t && rc == KZG_OK; first += group) {
        const size_t cnt = std::min(group, t - first);
        rc = combined_stage_unlocked(ctx, lk, s, coeffs, n, stride, first, cnt);
        if (rc == KZG_OK) rc = sets_passes(ctx, s, plan, s.cin.dev(), n, n, first, cnt, written);
    }
    return rc;
}
// h = sum_r Q(G_r, z_r) into s.q[0 .. n - 1) behind the passes (nothing for n < 2)
int sets_enqueue_scans(kzg_ctx* ctx, Slot& s, const SetsPlan& plan, size_t n) {
    if (n < 2) return KZG_OK;
    uint64_t ws[4 * KZG_MAX_SET_POINTS];  // (the weights are inside the G_r)
    for (size_t r = 0; r < plan.npts; r++) std::memcpy(ws + 4 * r, hf::kFrOne.l, 32);
    points_fill_roots(s.roots.h, plan.pts[0].l, ws, (uint32_t)plan.npts, (uint32_t)n);
    HIP_TRY(ctx, hipMemcpyAsync(s.roots.d, s.roots.h, plan.npts * points_root_bytes(), hipMemcpyHostToDevice, s.stream));
    if (s.timing) HIP_TRY(ctx, hipEventRecord(s.ev[6], s.stream));
    launch_quotient_sets(s.stream, s.sg.dev(), (uint32_t)n, s.roots.d, (uint32_t)plan.npts, s.q.dev(), s.pblock.dev(), s.pvals.dev());
    if (s.timing) HIP_TRY(ctx, hipEventRecord(s.ev[7], s.stream));
    HIP_TRY(ctx, hipGetLastError());
    return KZG_OK;
}
// the scans, the two tail checks on h (any coefficient at index >= srs_len: too high; any coefficient at all: else infinity)
// and the MSM over h
int sets_enqueue_open(kzg_ctx* ctx, Slot& s, const SetsPlan& plan, size_t n) {
    s.job_n = n;
    s.job_batch = 1;
    s.has_quotient = true;
    s.tail_checked = false;
    s.pts_nq = 0;
    s.sets_vmap = plan.vmap;
    std::memset(s.small.host(), 0, 64 * 4);  // (nothing in flight writes them: the passes do not touch the flag words)
    if (n >= 2) {
        int rc = sets_enqueue_scans(ctx, s, plan, n);
        if (rc) return rc;
        size_t nq = n - 1;
        if (nq > ctx->n) {
            const uint64_t cnt = nq - ctx->n;
            hipLaunchKernelGGL(k_tail_nonzero, dim3((unsigned)((cnt + 255) / 256)), dim3(256), 0, s.stream, s.q.dev(), (uint64_t)ctx->n,
                               (uint64_t)nq, s.small.dev() + 24);
            nq = ctx->n;
        }
        hipLaunchKernelGGL(k_tail_nonzero, dim3((unsigned)((nq + 255) / 256)), dim3(256), 0, s.stream, s.q.dev(), (uint64_t)0,
                           (uint64_t)nq, s.small.dev());
        int rc2 = enqueue_msm(ctx, s, s.q.dev(), 1, nq, 0);
        if (rc2) return rc2;
        s.pts_nq = nq;
    }
    HIP_TRY(ctx, hipEventRecord(s.done, s.end));
    s.kind = SLOT_OPEN_SETS;
    return KZG_OK;
}
void sets_copy_values(const Slot& s, uint64_t* out_ys) {
    for (size_t e = 0; e < s.sets_vmap.size(); e++) std::memcpy(out_ys + 4 * e, s.svals.host() + 8 * (size_t)s.sets_vmap[e], 32);
}

int wait_sets_locked(kzg_ctx* ctx, int slot, uint64_t* out_ys, uint64_t out_p1[18]) {
    if (slot < 0 || slot >= kNumSlots) return KZG_ERR_INVALID_ARG;
    Slot& s = ctx->slots[slot];
    if (s.kind == SLOT_RESERVED) return KZG_ERR_BUSY;  // a synchronous call on another thread owns it
    if (s.kind != SLOT_OPEN_SETS) {
        if (s.kind != SLOT_IDLE) ctx->last_error = "kzg_wait_sets on a slot that holds another kind of job";
        return KZG_ERR_INVALID_ARG;  // the job stays in the slot
    }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    slot_idle(ctx, s);
    HIP_TRY(ctx, hipEventSynchronize(s.done));
    const bool ran_msm = s.pts_nq > 0;
    if (ran_msm) fill_device_times(s);
    if (s.timing && s.job_n > 0) {
        float ms = 0;
        if (hipEventElapsedTime(&ms, s.cmb_ev[0], s.cmb_ev[1]) == hipSuccess) s.combine_ms = ms;
        if (ran_msm) {
            hipEventElapsedTime(&ms, s.ev[0], s.ev[1]); s.times.digits_ms = ms;
            hipEventElapsedTime(&ms, s.ev[2], s.ev[3]); s.times.scatter_ms = ms;
            fill_accumulate_times(s);
            hipEventElapsedTime(&ms, s.ev[4], s.ev[5]); s.times.reduce_ms = ms;
            hipEventElapsedTime(&ms, s.ev[6], s.ev[7]); s.times.quotient_ms = ms;
            hipEventElapsedTime(&ms, s.ev[6], s.ev[5]); s.times.total_ms = ms;
        }
    }
    sets_copy_values(s, out_ys);
    const uint32_t* hs = s.small.host();
    if (hs[24]) return KZG_ERR_DEGREE_TOO_HIGH;
    write_p1(out_p1, ran_msm && (hs[0] & 1u) ? finish_msm(ctx, s) : hf::p1_inf());  // h = 0 (also by cancellation): infinity
    return KZG_OK;
}
}  // namespace

int kzg_open_sets(kzg_ctx* ctx, const uint64_t* coeffs, size_t n, size_t t, size_t stride, const uint32_t* set_of,
                  const uint32_t* set_len, size_t m, const uint64_t* zs, const uint64_t gamma[4], uint64_t* out_ys,
                  uint64_t out_p1[18]) {
    if (!ctx) return KZG_ERR_INVALID_ARG;
    if (!set_of || !set_len || !zs || !gamma || !out_ys || !out_p1) {
        if (!ctx->multi) ctx->last_error = "kzg_open_sets: a null pointer";
        return KZG_ERR_INVALID_ARG;
    }
    SetsPlan plan;
    std::unique_lock<std::mutex> lk(ctx->mu);
    int rc = sets_check(ctx, "kzg_open_sets", coeffs, n, t, stride, set_of, set_len, m, zs, gamma, plan);
    if (rc) return rc;
    if (ctx->multi) {
        ctx->last_error.clear();  // (kzg_last_error then reads the devices' side)
        lk.unlock();
        return multi_open_sets(ctx->multi, coeffs, n, t, stride, set_of, set_len, m, zs, gamma, out_ys, out_p1);
    }
    if (!ctx->n || !ctx->slots_ready) return KZG_ERR_NO_SRS;
    const int slot = reserve_slot(ctx, lk, true);
    if (slot < 0) return KZG_ERR_BUSY;
    Slot& s = ctx->slots[slot];
    rc = sets_job_start(ctx, s, plan);
    if (rc == KZG_OK && n) rc = sets_host_passes(ctx, lk, s, plan, coeffs, n, stride);
    if (rc == KZG_OK) rc = sets_enqueue_open(ctx, s, plan, n);
    if (rc == KZG_OK) {
        await_unlocked(lk, s);
        rc = wait_sets_locked(ctx, slot, out_ys, out_p1);
    }
    release_owned(ctx, slot);
    return rc;
}

int kzg_open_sets_submit(kzg_ctx* ctx, int slot, const void* d_coeffs, size_t n, size_t t, size_t stride, const uint32_t* set_of,
                         const uint32_t* set_len, size_t m, const uint64_t* zs, const uint64_t gamma[4]) {
    KZG_SINGLE_DEVICE_ONLY(ctx);
    if (!ctx) return KZG_ERR_INVALID_ARG;
    if (!set_of || !set_len || !zs || !gamma) {
        ctx->last_error = "kzg_open_sets_submit: a null pointer";
        return KZG_ERR_INVALID_ARG;
    }
    SetsPlan plan;
    std::lock_guard<std::mutex> lk(ctx->mu);
    int rc = sets_check(ctx, "kzg_open_sets_submit", d_coeffs, n, t, stride, set_of, set_len, m, zs, gamma, plan);
    if (rc) return rc;
    if (!ctx->n || !ctx->slots_ready) return KZG_ERR_NO_SRS;
    if (slot < 0 || slot >= kNumSlots) return KZG_ERR_INVALID_ARG;
    Slot& s = ctx->slots[slot];
    if (s.kind != SLOT_IDLE) return KZG_ERR_BUSY;
    rc = sets_job_start(ctx, s, plan);
    if (rc == KZG_OK && n) {  // every pass takes all its polynomials in one launch
        bool written[KZG_MAX_SET_POINTS] = {};
        rc = sets_ensure_all(ctx, s, plan, n, t, 0);
        if (rc == KZG_OK) rc = sets_upload_tables(ctx, s, plan);
        if (rc == KZG_OK) rc = sets_passes(ctx, s, plan, (const uint32_t*)d_coeffs, n, stride, 0, t, written);
    }
    if (rc == KZG_OK) rc = sets_enqueue_open(ctx, s, plan, n);
    return rc;
}

int kzg_wait_sets(kzg_ctx* ctx, int slot, uint64_t* out_ys, uint64_t out_p1[18]) {
    KZG_SINGLE_DEVICE_ONLY(ctx);
    if (!ctx || !out_ys || !out_p1) return KZG_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(ctx->mu);
    return wait_sets_locked(ctx, slot, out_ys, out_p1);
}

int kzg_quotient_sets(kzg_ctx* ctx, const uint64_t* coeffs, size_t n, size_t t, size_t stride, const uint32_t* set_of,
                      const uint32_t* set_len, size_t m, const uint64_t* zs, const uint64_t gamma[4], uint64_t* out_ys,
                      uint64_t* out_h, size_t* out_hn) {
    if (!ctx) return KZG_ERR_INVALID_ARG;
    if (ctx->multi)  // needs no SRS
        return kzg_quotient_sets(multi_kid(ctx->multi, 0), coeffs, n, t, stride, set_of, set_len, m, zs, gamma, out_ys, out_h, out_hn);
    if (!set_of || !set_len || !zs || !gamma || !out_ys || !out_hn || (!out_h && n > 1)) {
        ctx->last_error = "kzg_quotient_sets: a null pointer";
        return KZG_ERR_INVALID_ARG;
    }
    SetsPlan plan;
    std::unique_lock<std::mutex> lk(ctx->mu);
    int rc = sets_check(ctx, "kzg_quotient_sets", coeffs, n, t, stride, set_of, set_len, m, zs, gamma, plan);
    if (rc) return rc;
    std::memset(out_ys, 0, 32 * plan.nvals);
    *out_hn = 0;
    if (n == 0) return KZG_OK;
    const int slot = reserve_slot(ctx, lk, true);
    if (slot < 0) return KZG_ERR_BUSY;
    SlotLease lease{ctx, slot};
    Slot& s = ctx->slots[slot];
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    rc = ensure_slot_basics(ctx, s);
    if (rc == KZG_OK) rc = sets_job_start(ctx, s, plan);
    if (rc == KZG_OK) rc = sets_host_passes(ctx, lk, s, plan, coeffs, n, stride);
    if (rc == KZG_OK) rc = sets_enqueue_scans(ctx, s, plan, n);
    if (rc) return rc;
    HIP_TRY(ctx, hipStreamSynchronize(s.stream));
    s.sets_vmap = plan.vmap;
    sets_copy_values(s, out_ys);
    if (n > 1) {
        HIP_TRY(ctx, hipMemcpy(out_h, s.q.dev(), (n - 1) * 32, hipMemcpyDeviceToHost));
        size_t hn = n - 1;
        while (hn > 0 && !(out_h[4 * hn - 4] | out_h[4 * hn - 3] | out_h[4 * hn - 2] | out_h[4 * hn - 1])) hn--;
        *out_hn = hn;
    }
    return KZG_OK;
}

// ---- host-pointer batches (BASELINE config 5: many openings against one SRS) ----------------------------------------
namespace {
struct BatchInFlight {
    int slot;
    size_t first_poly, polys;  // position in the caller's (first, step, count) sequence
};
// polynomials per submit: four or more sub-batches per call, so that the upload of one overlaps the kernels of the
// previous ones (a degree-2^20 polynomial is 32 MiB of pageable host memory), each at most max_batch polynomials -- and
// no more than ~2^19 terms: large polynomials go through the slots one by one, which is how the kernels of one overlap
// the accumulation of another (8 degree-2^20 openings per call: 378-382 /s in eight parts, 360 in four, 333 in two)
size_t host_batch_chunk(const kzg_ctx* ctx, size_t count, size_t n) {
    size_t chunk = (count + 3) / 4;
    const size_t by_size = n >= ((size_t)1 << 19) ? 1 : ((size_t)1 << 19) / (n ? n : 1);
    if (chunk > by_size) chunk = by_size;
    if (chunk > ctx->max_batch) chunk = ctx->max_batch;
    return chunk < 1 ? 1 : chunk;
}
}  // namespace

}  // extern "C"

namespace kzg {

int ctx_drop_srs(kzg_ctx* ctx) {
    std::unique_lock<std::mutex> lk(ctx->mu);
    if (!ctx->n && !ctx->table.p) return KZG_OK;
    quiesce(ctx, lk);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    return srs_release(ctx);
}

void ctx_set_raw_partials(kzg_ctx* ctx, bool raw) {
    std::lock_guard<std::mutex> lk(ctx->mu);
    ctx->raw_partials = raw;
}

// shared body of the two host-pointer batches: zs == nullptr -> commitments (lagrange: of values, over the held Lagrange basis)
static int batch_host(kzg_ctx* ctx, const uint64_t* coeffs, size_t n, size_t stride, size_t first, size_t step, size_t count,
                      const uint64_t* zs, const uint64_t* ys, uint64_t* out_p1s, int* statuses, bool lagrange = false) {
    if (!count) return KZG_OK;
    const bool opening = zs != nullptr;
    std::unique_lock<std::mutex> lk(ctx->mu);
    if (!ctx->n || !ctx->slots_ready) return KZG_ERR_NO_SRS;
    if ((opening ? n - 1 : n) > ctx->n) return KZG_ERR_DEGREE_TOO_HIGH;  // batches take truncated polynomials only
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t chunk = host_batch_chunk(ctx, count, n);
    std::deque<BatchInFlight> fifo;
    auto collect_oldest = [&]() -> int {
        const BatchInFlight b = fifo.front();
        fifo.pop_front();
        Slot& s = ctx->slots[b.slot];
        await_unlocked(lk, s);
        uint64_t* out = out_p1s + 18 * (first + b.first_poly * step);
        const int r = opening ? wait_open_batch_locked(ctx, b.slot, out, statuses + (first + b.first_poly * step), b.polys, 18 * step, step)
                              : wait_batch_locked(ctx, b.slot, out, b.polys, 18 * step);
        release_owned(ctx, b.slot);
        return r;
    };
    int rc = KZG_OK;
    std::vector<uint64_t> zc, yc;
    for (size_t at = 0; at < count && rc == KZG_OK; at += chunk) {
        const size_t polys = count - at < chunk ? count - at : chunk;
        int slot = reserve_slot(ctx, lk, false);
        while (slot < 0 && rc == KZG_OK) {
            if (!fifo.empty()) rc = collect_oldest();           // my own oldest sub-batch frees a slot
            else if ((slot = reserve_slot(ctx, lk, true)) < 0) rc = KZG_ERR_BUSY;  // other callers hold them all
            if (slot < 0 && rc == KZG_OK) slot = reserve_slot(ctx, lk, false);
        }
        if (rc != KZG_OK) {
            if (slot >= 0) release_owned(ctx, slot);
            break;
        }
        Slot& s = ctx->slots[slot];
        rc = ensure_poly(ctx, s, n * polys);
        for (size_t q = 0; q < polys && rc == KZG_OK; q++)
            rc = upload_unlocked(ctx, lk, s, s.stage.dev() + (q * n) * 8, coeffs + (first + (at + q) * step) * stride * 4, n * 32);
        if (rc == KZG_OK) {
            if (opening) {
                zc.resize(4 * polys);
                yc.resize(4 * polys);
                for (size_t q = 0; q < polys; q++) {
                    std::memcpy(&zc[4 * q], zs + 4 * (first + (at + q) * step), 32);
                    std::memcpy(&yc[4 * q], ys + 4 * (first + (at + q) * step), 32);
                }
                rc = open_batch_submit_locked(ctx, slot, s.stage.dev(), n, polys, n, zc.data(), yc.data(), true);
            } else {
                rc = commit_batch_submit_locked(ctx, slot, s.stage.dev(), n, polys, n, true, lagrange);
            }
        }
        if (rc != KZG_OK) {
            release_owned(ctx, slot);
            break;
        }
        fifo.push_back({slot, at, polys});
    }
    while (!fifo.empty()) {
        const int r = collect_oldest();
        if (rc == KZG_OK) rc = r;
    }
    return rc;
}

int ctx_commit_batch_host(kzg_ctx* ctx, const uint64_t* coeffs, size_t n, size_t stride_coeffs, size_t first, size_t step,
                          size_t count, uint64_t* out_p1s) {
    return batch_host(ctx, coeffs, n, stride_coeffs, first, step, count, nullptr, nullptr, out_p1s, nullptr);
}
int ctx_open_batch_host(kzg_ctx* ctx, const uint64_t* coeffs, size_t n, size_t stride_coeffs, size_t first, size_t step,
                        size_t count, const uint64_t* zs, const uint64_t* ys, uint64_t* out_p1s, int* statuses) {
    return batch_host(ctx, coeffs, n, stride_coeffs, first, step, count, zs, ys, out_p1s, statuses);
}
static int commit_lagrange_batch_host(kzg_ctx* ctx, const uint64_t* evals, size_t n, size_t stride, size_t count, uint64_t* out_p1s) {
    return batch_host(ctx, evals, n, stride, 0, 1, count, nullptr, nullptr, out_p1s, nullptr, true);
}

// ---- one device's share of a range-sharded opening: the slice is staged once (multi.hip) ----------------------------
int ctx_open_slice_begin(kzg_ctx* ctx, const uint64_t* slice, size_t len, const uint64_t z[4], uint64_t out_h[4], int* slot_out) {
    std::unique_lock<std::mutex> lk(ctx->mu);
    if (!ctx->n || !ctx->slots_ready) return KZG_ERR_NO_SRS;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const int slot = reserve_slot(ctx, lk, true);
    if (slot < 0) return KZG_ERR_BUSY;
    Slot& s = ctx->slots[slot];
    int rc = ensure_poly(ctx, s, len + 1);
    if (rc == KZG_OK) rc = upload_unlocked(ctx, lk, s, s.stage.dev(), slice, len * 32);
    if (rc == KZG_OK) {
        lk.unlock();
        uint32_t zw[8];
        std::memcpy(zw, z, 32);
        std::memset(s.small.host(), 0, 64 * 4);
        hipError_t e = hipSuccess;
        PolyScratch sc{s.chunk.dev(), s.block.dev(), s.small.dev(), s.small.dev() + 8};
        launch_quotient(s.stream, s.stage.dev(), (uint32_t)len, zw, nullptr, sc);
        if (e == hipSuccess) e = hipGetLastError();
        if (e == hipSuccess) e = hipStreamSynchronize(s.stream);
        lk.lock();
        if (e != hipSuccess) {
            ctx->last_error = std::string("slice evaluation: ") + hipGetErrorString(e);
            rc = KZG_ERR_HIP;
        }
    }
    if (rc != KZG_OK) {
        release_owned(ctx, slot);
        return rc;
    }
    std::memcpy(out_h, s.small.host() + 8, 32);
    *slot_out = slot;
    return KZG_OK;
}

int ctx_open_slice_finish(kzg_ctx* ctx, int slot, size_t len, const uint64_t carry[4], const uint64_t z[4],
                          const uint64_t start[4], uint64_t out_p1[18]) {
    std::unique_lock<std::mutex> lk(ctx->mu);
    Slot& s = ctx->slots[slot];
    int rc = KZG_OK;
    if (hipSetDevice(ctx->device) != hipSuccess) rc = KZG_ERR_HIP;
    if (rc == KZG_OK) rc = copy_unlocked(ctx, lk, s.stream, s.stage.dev() + len * 8, carry, 1 * 32, hipMemcpyHostToDevice, kCopyCoeffs);  // the carry as one more top coefficient
    if (rc == KZG_OK) rc = submit_open_locked(ctx, slot, s.stage.dev(), len + 1, z, start, true);
    if (rc == KZG_OK) {
        await_unlocked(lk, s);
        rc = wait_locked(ctx, slot, out_p1);
    }
    release_owned(ctx, slot);
    return rc;
}

void ctx_open_slice_abort(kzg_ctx* ctx, int slot) {
    std::lock_guard<std::mutex> lk(ctx->mu);
    release_owned(ctx, slot);
}

}  // namespace kzg

extern "C" {

int kzg_commit_batch(kzg_ctx* ctx, const uint64_t* coeffs, size_t n, size_t batch, size_t stride_coeffs, uint64_t* out_p1s) {
    if (!ctx || (!coeffs && batch) || (!out_p1s && batch) || n == 0 || stride_coeffs < n || n > kMaxCoefficients) return KZG_ERR_INVALID_ARG;
    if (ctx->multi) return multi_commit_batch(ctx->multi, coeffs, n, batch, stride_coeffs, out_p1s);
    return ctx_commit_batch_host(ctx, coeffs, n, stride_coeffs, 0, 1, batch, out_p1s);
}

int kzg_open_batch(kzg_ctx* ctx, const uint64_t* coeffs, size_t n, size_t batch, size_t stride_coeffs, const uint64_t* zs,
                   const uint64_t* ys, uint64_t* out_p1s, int* statuses) {
    if (!ctx || ((!coeffs || !zs || !ys || !out_p1s || !statuses) && batch) || stride_coeffs < n || n > kMaxCoefficients)
        return KZG_ERR_INVALID_ARG;
    if (n < 2) {  // empty and constant polynomials: the single-opening path knows their rules (src/polynomial.rs:138-167)
        for (size_t p = 0; p < batch; p++) {
            const int rc = kzg_open(ctx, coeffs + p * stride_coeffs * 4, n, zs + 4 * p, ys + 4 * p, out_p1s + 18 * p);
            if (rc != KZG_OK && rc != KZG_ERR_CONSTANT_POLY && rc != KZG_ERR_REMAINDER && rc != KZG_ERR_DEGREE_TOO_HIGH) return rc;
            statuses[p] = rc;
        }
        return KZG_OK;
    }
    if (ctx->multi) return multi_open_batch(ctx->multi, coeffs, n, batch, stride_coeffs, zs, ys, out_p1s, statuses);
    return ctx_open_batch_host(ctx, coeffs, n, stride_coeffs, 0, 1, batch, zs, ys, out_p1s, statuses);
}

int kzg_quotient(kzg_ctx* ctx, const uint64_t* coeffs, size_t n, const uint64_t z[4], const uint64_t y[4],
                 uint64_t* out_q, size_t* out_qn) {
    if (!ctx || !z || !y || !out_qn || (!coeffs && n) || (!out_q && n > 1)) return KZG_ERR_INVALID_ARG;
    if (n > kMaxCoefficients) return KZG_ERR_INVALID_ARG;
    if (ctx->multi) return kzg_quotient(multi_kid(ctx->multi, 0), coeffs, n, z, y, out_q, out_qn);  // needs no SRS
    std::unique_lock<std::mutex> lk(ctx->mu);
    *out_qn = 0;
    const int slot = reserve_slot(ctx, lk, true);
    if (slot < 0) return KZG_ERR_BUSY;
    SlotLease lease{ctx, slot};
    Slot& s = ctx->slots[slot];
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    int rcb = ensure_slot_basics(ctx, s);  // quotient does not need an SRS
    if (rcb) return rcb;
    bool y_zero = (y[0] | y[1] | y[2] | y[3]) == 0;
    if (n == 0) return y_zero ? KZG_OK : KZG_ERR_CONSTANT_POLY;
    int rc = ensure_poly(ctx, s, n);
    if (rc) return rc;
    HIP_TRY(ctx, hipMemcpyAsync(s.stage.dev(), coeffs, n * 32, hipMemcpyHostToDevice, s.stream));
    std::memset(s.small.host(), 0, 64 * 4);
    uint32_t zw[8];
    std::memcpy(zw, z, 32);
    PolyScratch sc{s.chunk.dev(), s.block.dev(), s.small.dev(), s.small.dev() + 8};
    launch_quotient(s.stream, s.stage.dev(), (uint32_t)n, zw, n > 1 ? s.q.dev() : nullptr, sc);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipStreamSynchronize(s.stream));
    bool higher_nonzero = s.small.host()[0] & 1u;
    if (!higher_nonzero) return std::memcmp(coeffs, y, 32) == 0 ? KZG_OK : KZG_ERR_CONSTANT_POLY;
    if (std::memcmp(s.small.host() + 8, y, 32) != 0) return KZG_ERR_REMAINDER;
    // quotient of the truncated polynomial: its length is (index of the last non-zero coefficient)
    size_t n_eff = n;
    while (n_eff > 1 && !(coeffs[4 * (n_eff - 1)] | coeffs[4 * (n_eff - 1) + 1] | coeffs[4 * (n_eff - 1) + 2] |
                          coeffs[4 * (n_eff - 1) + 3]))
        n_eff--;
    HIP_TRY(ctx, hipMemcpy(out_q, s.q.dev(), (n_eff - 1) * 32, hipMemcpyDeviceToHost));
    *out_qn = n_eff - 1;
    return KZG_OK;
}

int kzg_evaluate(kzg_ctx* ctx, const uint64_t* coeffs, size_t n, const uint64_t z[4], uint64_t out_y[4]) {
    if (!ctx || !z || !out_y || (!coeffs && n)) return KZG_ERR_INVALID_ARG;
    if (n > kMaxCoefficients) return KZG_ERR_INVALID_ARG;
    if (ctx->multi) return kzg_evaluate(multi_kid(ctx->multi, 0), coeffs, n, z, out_y);  // needs no SRS
    std::unique_lock<std::mutex> lk(ctx->mu);
    std::memset(out_y, 0, 32);
    if (n == 0) return KZG_OK;
    const int slot = reserve_slot(ctx, lk, true);
    if (slot < 0) return KZG_ERR_BUSY;
    SlotLease lease{ctx, slot};
    Slot& s = ctx->slots[slot];
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    int rcb = ensure_slot_basics(ctx, s);
    if (rcb) return rcb;
    int rc = ensure_poly(ctx, s, n);
    if (rc) return rc;
    HIP_TRY(ctx, hipMemcpyAsync(s.stage.dev(), coeffs, n * 32, hipMemcpyHostToDevice, s.stream));
    std::memset(s.small.host(), 0, 64 * 4);
    uint32_t zw[8];
    std::memcpy(zw, z, 32);
    PolyScratch sc{s.chunk.dev(), s.block.dev(), s.small.dev(), s.small.dev() + 8};
    launch_quotient(s.stream, s.stage.dev(), (uint32_t)n, zw, nullptr, sc);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipStreamSynchronize(s.stream));
    std::memcpy(out_y, s.small.host() + 8, 32);
    return KZG_OK;
}

// the multiproof scan alone on a slot of the context (no SRS needed): coefficients uploaded, values (and q) computed,
// the stream drained.  Claims and truncation are the caller's business.
static int points_scan_host(kzg_ctx* ctx, Slot& s, const uint64_t* coeffs, size_t n, const uint64_t* zs, size_t k, bool want_q) {
    uint64_t ws[4 * KZG_MAX_OPEN_POINTS];
    int rc = points_weights(ctx, zs, k, ws);
    if (rc) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    rc = ensure_slot_basics(ctx, s);
    if (rc == KZG_OK) rc = ensure_poly(ctx, s, n);
    if (rc == KZG_OK) rc = ensure_points(ctx, s, n, k);
    if (rc) return rc;
    if (n) HIP_TRY(ctx, hipMemcpyAsync(s.stage.dev(), coeffs, n * 32, hipMemcpyHostToDevice, s.stream));
    rc = enqueue_points_scan(ctx, s, s.stage.dev(), n, zs, ws, k, n > k ? n - k : 0, want_q && n > k);
    if (rc) return rc;
    HIP_TRY(ctx, hipStreamSynchronize(s.stream));
    return KZG_OK;
}

int kzg_quotient_points(kzg_ctx* ctx, const uint64_t* coeffs, size_t n, const uint64_t* zs, const uint64_t* ys, size_t k,
                        uint64_t* out_q, size_t* out_qn) {
    if (!ctx || !zs || !ys || !out_qn || (!coeffs && n) || (!out_q && n > k) || n > kMaxCoefficients) return KZG_ERR_INVALID_ARG;
    if (ctx->multi) return kzg_quotient_points(multi_kid(ctx->multi, 0), coeffs, n, zs, ys, k, out_q, out_qn);  // needs no SRS
    std::unique_lock<std::mutex> lk(ctx->mu);
    *out_qn = 0;
    const int slot = reserve_slot(ctx, lk, true);
    if (slot < 0) return KZG_ERR_BUSY;
    SlotLease lease{ctx, slot};
    Slot& s = ctx->slots[slot];
    int rc = points_scan_host(ctx, s, coeffs, n, zs, k, true);
    if (rc) return rc;
    const uint32_t* vals = points_values(s, k);
    for (size_t i = 0; i < k; i++)
        if (std::memcmp(vals + 8 * i, ys + 4 * i, 32) != 0) return KZG_ERR_REMAINDER;
    // q of the truncated polynomial: n' - k coefficients (none when n' <= k)
    size_t n_eff = n;
    while (n_eff > 0 && !(coeffs[4 * (n_eff - 1)] | coeffs[4 * (n_eff - 1) + 1] | coeffs[4 * (n_eff - 1) + 2] |
                          coeffs[4 * (n_eff - 1) + 3]))
        n_eff--;
    if (n_eff <= k) return KZG_OK;
    HIP_TRY(ctx, hipMemcpy(out_q, s.q.dev(), (n_eff - k) * 32, hipMemcpyDeviceToHost));
    *out_qn = n_eff - k;
    return KZG_OK;
}

int kzg_evaluate_points(kzg_ctx* ctx, const uint64_t* coeffs, size_t n, const uint64_t* zs, size_t k, uint64_t* out_ys) {
    if (!ctx || !zs || !out_ys || (!coeffs && n) || n > kMaxCoefficients) return KZG_ERR_INVALID_ARG;
    if (ctx->multi) return kzg_evaluate_points(multi_kid(ctx->multi, 0), coeffs, n, zs, k, out_ys);  // needs no SRS
    std::unique_lock<std::mutex> lk(ctx->mu);
    const int slot = reserve_slot(ctx, lk, true);
    if (slot < 0) return KZG_ERR_BUSY;
    SlotLease lease{ctx, slot};
    Slot& s = ctx->slots[slot];
    int rc = points_scan_host(ctx, s, coeffs, n, zs, k, false);
    if (rc) return rc;
    std::memcpy(out_ys, points_values(s, k), 32 * k);
    return KZG_OK;
}

// ---- polynomials in evaluation form (NTT over power-of-two domains) -------------------------------------------------

// log2 n for a domain size the transform supports (a power of two up to 2^22); false otherwise
static bool ntt_log(size_t n, uint32_t* lg) {
    if (n == 0 || (n & (n - 1)) || n > ((size_t)1 << kNttMaxLog)) return false;
    uint32_t k = 0;
    while (((size_t)1 << k) < n) k++;
    *lg = k;
    return true;
}
// the context's twiddle tables (ctx->mu held): one set for every size, w = w_(2^22) and its inverse, 4 x 2048 Fr30
// (the caller has made ctx->device current, as for everything that allocates or launches below)
static int ensure_ntt(kzg_ctx* ctx) {
    if (ctx->ntt_tw.p) return KZG_OK;
    if (!ntt_prepare_device()) {
        (void)hipGetLastError();
        ctx->last_error = "ntt: the pass kernel's LDS limit could not be raised";
        return KZG_ERR_HIP;
    }
    std::vector<Fr30> h(4 * kNttTableLen);
    const hf::Fr w = hf::fr_domain_root(kNttMaxLog);
    for (int dir = 0; dir < 2; dir++) {
        const hf::Fr base = dir ? hf::fr_inv(w) : w;
        const hf::Fr step_hi = hf::fr_pow(base, kNttTableLen);
        hf::Fr lo = hf::kFrOne, hi = hf::kFrOne;
        for (uint32_t i = 0; i < kNttTableLen; i++) {
            h[2 * dir * kNttTableLen + i] = fr30_arg_from_mont256(lo);
            h[(2 * dir + 1) * kNttTableLen + i] = fr30_arg_from_mont256(hi);
            lo = hf::fr_mul(lo, base);
            hi = hf::fr_mul(hi, step_hi);
        }
    }
    DevBuf d;
    HIP_TRY(ctx, hipMalloc(&d.p, h.size() * sizeof(Fr30)));
    if (hipError_t e = hipMemcpy(d.p, h.data(), h.size() * sizeof(Fr30), hipMemcpyHostToDevice))
        return hip_fail(ctx, "hipMemcpy (ntt twiddles)", e);
    std::swap(ctx->ntt_tw.p, d.p);
    return KZG_OK;
}
// enqueues the transform of 2^lg values on stream st: d_in -> d_out through the scratch buffers a, b (launch_ntt)
static int enqueue_ntt(kzg_ctx* ctx, hipStream_t st, const uint32_t* d_in, uint32_t* d_out, uint32_t lg, bool inverse,
                       uint32_t* d_a, uint32_t* d_b) {
    hf::Fr c = hf::kFrOne;  // the last pass's multiplier: 1, or 1/n
    if (inverse) {
        hf::Fr n = hf::kFrOne;
        for (uint32_t i = 0; i < lg; i++) n = hf::fr_add(n, n);
        c = hf::fr_inv(n);
    }
    const Fr30 last_c = fr30_arg_from_mont256(c);
    const Fr30* tw = (const Fr30*)ctx->ntt_tw.p + (inverse ? 2 * kNttTableLen : 0);
    launch_ntt(st, d_in, d_out, lg, tw, last_c, d_a, d_b);
    HIP_TRY(ctx, hipGetLastError());
    return KZG_OK;
}
// Transforms that end in a slot's staging buffer use the slot's two polynomial buffers as the pass chain: with three
// passes the chain is q -> stage -> q -> stage, otherwise stage (-> q) -> stage.  Host data goes in at ntt_slot_input.
static uint32_t* ntt_slot_input(Slot& s, uint32_t lg) { return ntt_plan(lg).passes == 3 ? s.q.dev() : s.stage.dev(); }
static int ntt_into_stage(kzg_ctx* ctx, Slot& s, const uint32_t* d_in, uint32_t lg, bool inverse) {
    const bool three = ntt_plan(lg).passes == 3;
    return enqueue_ntt(ctx, s.stream, d_in, s.stage.dev(), lg, inverse, three ? s.stage.dev() : s.q.dev(), s.q.dev());
}
// a slot reserved by the caller, ready for a transform of n values (ctx->mu held, twiddles built)
static int ntt_slot_ready(kzg_ctx* ctx, Slot& s, size_t n) {
    int rc = ensure_slot_basics(ctx, s);
    if (rc == KZG_OK) rc = ensure_poly(ctx, s, n);
    return rc;
}

int kzg_domain_root(unsigned log_n, uint64_t out_mont[4]) {
    if (!out_mont || log_n > 32) return KZG_ERR_INVALID_ARG;
    const hf::Fr w = hf::fr_domain_root(log_n);
    std::memcpy(out_mont, w.l, 32);
    return KZG_OK;
}

int kzg_ntt(kzg_ctx* ctx, const uint64_t* in, size_t n, int inverse, uint64_t* out) {
    uint32_t lg = 0;
    if (!ctx || !in || !out || !ntt_log(n, &lg)) return KZG_ERR_INVALID_ARG;
    if (ctx->multi) return kzg_ntt(multi_kid(ctx->multi, 0), in, n, inverse, out);  // needs no SRS
    std::unique_lock<std::mutex> lk(ctx->mu);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    int rc = ensure_ntt(ctx);
    if (rc) return rc;
    const int slot = reserve_slot(ctx, lk, true);
    if (slot < 0) return KZG_ERR_BUSY;
    SlotLease lease{ctx, slot};
    Slot& s = ctx->slots[slot];
    rc = ntt_slot_ready(ctx, s, n);
    if (rc) return rc;
    HIP_TRY(ctx, hipMemcpyAsync(ntt_slot_input(s, lg), in, n * 32, hipMemcpyHostToDevice, s.stream));
    rc = ntt_into_stage(ctx, s, ntt_slot_input(s, lg), lg, inverse != 0);
    if (rc) return rc;
    HIP_TRY(ctx, hipMemcpyAsync(out, s.stage.dev(), n * 32, hipMemcpyDeviceToHost, s.stream));
    HIP_TRY(ctx, hipStreamSynchronize(s.stream));
    return KZG_OK;
}

int kzg_ntt_device(kzg_ctx* ctx, const void* d_in, void* d_out, size_t n, int inverse) {
    KZG_SINGLE_DEVICE_ONLY(ctx);
    uint32_t lg = 0;
    if (!ctx || !d_in || !d_out || !ntt_log(n, &lg)) return KZG_ERR_INVALID_ARG;
    std::unique_lock<std::mutex> lk(ctx->mu);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    int rc = ensure_ntt(ctx);
    if (rc) return rc;
    const int slot = reserve_slot(ctx, lk, true);
    if (slot < 0) return KZG_ERR_BUSY;
    SlotLease lease{ctx, slot};
    Slot& s = ctx->slots[slot];
    rc = ntt_slot_ready(ctx, s, n);
    if (rc) return rc;
    // the caller's buffers are neither of the slot's: d_in -> stage (-> q) -> d_out
    rc = enqueue_ntt(ctx, s.stream, (const uint32_t*)d_in, (uint32_t*)d_out, lg, inverse != 0, s.stage.dev(), s.q.dev());
    if (rc) return rc;
    HIP_TRY(ctx, hipStreamSynchronize(s.stream));
    return KZG_OK;
}

int kzg_commit_evaluations_submit(kzg_ctx* ctx, int slot, const void* d_evals, size_t n) {
    KZG_SINGLE_DEVICE_ONLY(ctx);
    uint32_t lg = 0;
    if (!ctx || !d_evals || !ntt_log(n, &lg)) return KZG_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(ctx->mu);
    if (!ctx->n || !ctx->slots_ready) return KZG_ERR_NO_SRS;
    if (slot < 0 || slot >= kNumSlots) return KZG_ERR_INVALID_ARG;
    Slot& s = ctx->slots[slot];
    if (s.kind != SLOT_IDLE) return KZG_ERR_BUSY;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    int rc = ensure_ntt(ctx);
    if (rc == KZG_OK) rc = ntt_slot_ready(ctx, s, n);
    if (rc == KZG_OK) rc = ntt_into_stage(ctx, s, (const uint32_t*)d_evals, lg, true);
    if (rc) return rc;
    // n above the SRS: the coefficients beyond it are checked on the device, as for kzg_commit_submit
    return submit_commit_locked(ctx, slot, s.stage.dev(), 1, n, false);
}

// the synchronous host-pointer forms: upload -> inverse NTT -> kzg_commit's / kzg_open's submit, on a reserved slot
static int evaluations_host(kzg_ctx* ctx, const uint64_t* evals, size_t n, uint32_t lg, const uint64_t* z, const uint64_t* y,
                            uint64_t out_p1[18]) {
    std::unique_lock<std::mutex> lk(ctx->mu);
    if (!ctx->n || !ctx->slots_ready) return KZG_ERR_NO_SRS;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    int rc = ensure_ntt(ctx);
    if (rc) return rc;
    const int slot = reserve_slot(ctx, lk, true);
    if (slot < 0) return KZG_ERR_BUSY;
    SlotLease lease{ctx, slot};
    Slot& s = ctx->slots[slot];
    rc = ntt_slot_ready(ctx, s, n);
    if (rc) return rc;
    uint32_t* dst = ntt_slot_input(s, lg);
    rc = copy_unlocked(ctx, lk, s.stream, dst, evals, n * 32, hipMemcpyHostToDevice, "hipMemcpyAsync (evaluations)");
    if (rc) return rc;
    rc = ntt_into_stage(ctx, s, dst, lg, true);
    if (rc) return rc;
    rc = z ? submit_open_locked(ctx, slot, s.stage.dev(), n, z, y, true)
           : submit_commit_locked(ctx, slot, s.stage.dev(), 1, n, false, true);
    if (rc) return rc;
    await_unlocked(lk, s);
    return wait_locked(ctx, slot, out_p1);
}
// a multi-device context: a replicated SRS forwards to one device, a range-split one cannot take a whole-domain transform
static kzg_ctx* evaluations_kid(kzg_ctx* ctx, int* rc) {
    if (multi_mode(ctx->multi) != kMultiReplicate) {
        *rc = KZG_ERR_INVALID_ARG;
        return nullptr;
    }
    if (!multi_srs_len(ctx->multi)) {
        *rc = KZG_ERR_NO_SRS;
        return nullptr;
    }
    return multi_kid(ctx->multi, 0);
}

int kzg_commit_evaluations(kzg_ctx* ctx, const uint64_t* evals, size_t n, uint64_t out_p1[18]) {
    uint32_t lg = 0;
    if (!ctx || !evals || !out_p1 || !ntt_log(n, &lg)) return KZG_ERR_INVALID_ARG;
    if (ctx->multi) {
        int rc = KZG_OK;
        kzg_ctx* kid = evaluations_kid(ctx, &rc);
        return kid ? kzg_commit_evaluations(kid, evals, n, out_p1) : rc;
    }
    return evaluations_host(ctx, evals, n, lg, nullptr, nullptr, out_p1);
}

int kzg_open_evaluations(kzg_ctx* ctx, const uint64_t* evals, size_t n, const uint64_t z[4], const uint64_t y[4],
                         uint64_t out_p1[18]) {
    uint32_t lg = 0;
    if (!ctx || !evals || !z || !y || !out_p1 || !ntt_log(n, &lg)) return KZG_ERR_INVALID_ARG;
    if (ctx->multi) {
        int rc = KZG_OK;
        kzg_ctx* kid = evaluations_kid(ctx, &rc);
        return kid ? kzg_open_evaluations(kid, evals, n, z, y, out_p1) : rc;
    }
    return evaluations_host(ctx, evals, n, lg, z, y, out_p1);
}

// ---- every cell of a domain and its multiproof (cell_kernels.hip) ---------------------------------
// Cell j of the domain of N = 2^log_n points is {w_N^(j + (N/l) i) : i < l}, l = 2^log_l; its proof is the commitment to
// q_j = (P - I_j) / (X^l - w_N^(j l)).  The call holds one slot for its whole length: P sits in that slot's cpoly, the cells
// come from its stream, and the N/l quotients flow through it and any other free slot in sub-batches of at most
// ctx->max_batch cells (one batched MSM each), the kernels of one sub-batch overlapping the MSMs of the others.
namespace {
struct CellsShape {
    uint32_t log_n = 0, log_l = 0;
    size_t N = 0, l = 0, cells = 0;
};
bool cells_shape(size_t n, unsigned log_domain, unsigned log_cell, CellsShape* sh) {
    if (log_domain > kNttMaxLog || log_cell > KZG_MAX_CELL_LOG || log_cell > log_domain) return false;
    sh->log_n = log_domain;
    sh->log_l = log_cell;
    sh->N = (size_t)1 << log_domain;
    sh->l = (size_t)1 << log_cell;
    sh->cells = sh->N >> log_cell;
    return n <= sh->N;
}
// n without trailing zero coefficients
size_t cells_trim(const uint64_t* c, size_t n) {
    while (n > 0 && !(c[4 * (n - 1)] | c[4 * (n - 1) + 1] | c[4 * (n - 1) + 2] | c[4 * (n - 1) + 3])) n--;
    return n;
}
}  // namespace

// the slot's buffer for P (cap coefficients) and its hand-off event (ctx->mu held, slot owned by the caller)
static int ensure_cells_poly(kzg_ctx* ctx, Slot& s, size_t cap) {
    if (!s.cells_ev) HIP_TRY(ctx, hipEventCreateWithFlags(&s.cells_ev, hipEventDisableTiming));
    return s.cpoly.reserve(ctx, (cap < 1024 ? 1024 : cap) * 32, s.stream);
}
// the quotients of cells [first, first + polys) on slot `slot` (owned), then their batched MSM; P in s0.cpoly
static int cells_submit(kzg_ctx* ctx, int slot, Slot& s0, const CellsShape& sh, size_t nq, size_t first, size_t polys) {
    Slot& s = ctx->slots[slot];
    int rc = ensure_poly(ctx, s, polys * nq);
    if (rc == KZG_OK) rc = s.cagg.reserve(ctx, cells_agg_words((uint32_t)nq, sh.log_l, (uint32_t)polys) * 4, s.stream);
    if (rc) return rc;
    if (&s != &s0) HIP_TRY(ctx, hipStreamWaitEvent(s.stream, s0.cells_ev, 0));
    launch_cell_quotients(s.stream, s0.cpoly.dev(), (uint32_t)nq, sh.log_n, sh.log_l, (uint32_t)first, (uint32_t)polys,
                          ctx->ntt_tw.p, s.cagg.dev(), s.q.dev(), nq);
    HIP_TRY(ctx, hipGetLastError());
    return commit_batch_submit_locked(ctx, slot, s.q.dev(), nq, polys, nq, true);
}
// P sits in s0.cpoly: n_eff coefficients, zero up to N when the cells are wanted.  Cells first, then the proofs.
static int cells_run(kzg_ctx* ctx, std::unique_lock<std::mutex>& lk, int slot0, const CellsShape& sh, size_t n_eff,
                     uint64_t* out_cells, uint64_t* out_proofs) {
    Slot& s0 = ctx->slots[slot0];
    HIP_TRY(ctx, hipEventRecord(s0.cells_ev, s0.stream));
    int rc = KZG_OK;
    if (out_cells) {
        // forward NTT of P padded to N (cpoly -> stage, through q), gathered into cell-major order in q
        rc = ensure_poly(ctx, s0, sh.N);
        if (rc == KZG_OK) rc = ntt_into_stage(ctx, s0, s0.cpoly.dev(), sh.log_n, false);
        if (rc) return rc;
        launch_cells_gather(s0.stream, s0.stage.dev(), s0.q.dev(), sh.log_n, sh.log_l);
        HIP_TRY(ctx, hipGetLastError());
        lk.unlock();
        hipError_t e = hipMemcpyAsync(out_cells, s0.q.dev(), sh.N * 32, hipMemcpyDeviceToHost, s0.stream);
        if (e == hipSuccess) e = hipStreamSynchronize(s0.stream);
        lk.lock();
        if (e != hipSuccess) {
            ctx->last_error = std::string("cells: ") + hipGetErrorString(e);
            return KZG_ERR_HIP;
        }
    }
    const size_t nq = n_eff > sh.l ? n_eff - sh.l : 0;
    if (!nq) {  // P has at most l coefficients: it is its own interpolant on every cell
        const hf::P1 inf = hf::p1_inf();
        for (size_t j = 0; j < sh.cells; j++) write_p1(out_proofs + 18 * j, inf);
        return KZG_OK;
    }
    const size_t chunk = host_batch_chunk(ctx, sh.cells, nq);
    std::deque<BatchInFlight> fifo;
    bool busy[kNumSlots] = {};
    // keep: the slot stays the caller's (SLOT_RESERVED) for the next sub-batch; slot0 always does
    auto collect_oldest = [&](bool keep) -> int {
        const BatchInFlight b = fifo.front();
        fifo.pop_front();
        Slot& s = ctx->slots[b.slot];
        await_unlocked(lk, s);
        const int r = wait_batch_locked(ctx, b.slot, out_proofs + 18 * b.first_poly, b.polys);
        busy[b.slot] = false;
        if (keep || b.slot == slot0) s.kind = SLOT_RESERVED;  // (the mutex was held since wait_batch_locked marked it idle)
        else release_owned(ctx, b.slot);
        return r;
    };
    for (size_t at = 0; at < sh.cells && rc == KZG_OK; at += chunk) {
        const size_t polys = sh.cells - at < chunk ? sh.cells - at : chunk;
        int slot = busy[slot0] ? reserve_slot(ctx, lk, false) : slot0;
        if (slot < 0) {
            slot = fifo.front().slot;
            rc = collect_oldest(true);
            if (rc) {
                if (slot != slot0) release_owned(ctx, slot);
                break;
            }
        }
        rc = cells_submit(ctx, slot, s0, sh, nq, at, polys);
        if (rc) {
            if (slot != slot0) release_owned(ctx, slot);
            break;
        }
        busy[slot] = true;
        fifo.push_back({slot, at, polys});
    }
    while (!fifo.empty()) {
        const int r = collect_oldest(false);
        if (rc == KZG_OK) rc = r;
    }
    return rc;
}
// the synchronous forms: P by coefficients (coeffs, n_eff trimmed) or by its values over the n-domain (evals, n)
static int cells_host(kzg_ctx* ctx, const uint64_t* coeffs, size_t n_eff, const uint64_t* evals, size_t n, const CellsShape& sh,
                      uint64_t* out_cells, uint64_t* out_proofs) {
    std::unique_lock<std::mutex> lk(ctx->mu);
    if (!ctx->n || !ctx->slots_ready) return KZG_ERR_NO_SRS;
    if (!evals && n_eff > sh.l && n_eff - sh.l > ctx->n) return KZG_ERR_DEGREE_TOO_HIGH;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    int rc = ensure_ntt(ctx);
    if (rc) return rc;
    const int slot0 = reserve_slot(ctx, lk, true);
    if (slot0 < 0) return KZG_ERR_BUSY;
    SlotLease lease{ctx, slot0};
    Slot& s0 = ctx->slots[slot0];
    rc = ensure_cells_poly(ctx, s0, sh.N);
    if (rc) return rc;
    if (evals) {
        // values -> cpoly -> inverse NTT into stage -> back to cpoly; the coefficients also go to the host once, for n'
        uint32_t lg = 0;
        (void)ntt_log(n, &lg);
        rc = ntt_slot_ready(ctx, s0, n);
        if (rc == KZG_OK) rc = copy_unlocked(ctx, lk, s0.stream, s0.cpoly.dev(), evals, n * 32, hipMemcpyHostToDevice, "hipMemcpyAsync (cells)");
        if (rc == KZG_OK) rc = ntt_into_stage(ctx, s0, s0.cpoly.dev(), lg, true);
        if (rc) return rc;
        HIP_TRY(ctx, hipMemcpyAsync(s0.cpoly.dev(), s0.stage.dev(), n * 32, hipMemcpyDeviceToDevice, s0.stream));
        std::vector<uint64_t> c(4 * n);
        lk.unlock();
        hipError_t e = hipMemcpyAsync(c.data(), s0.stage.dev(), n * 32, hipMemcpyDeviceToHost, s0.stream);
        if (e == hipSuccess) e = hipStreamSynchronize(s0.stream);
        lk.lock();
        if (e != hipSuccess) {
            ctx->last_error = std::string("cells (interpolation): ") + hipGetErrorString(e);
            return KZG_ERR_HIP;
        }
        n_eff = cells_trim(c.data(), n);
        if (n_eff > sh.l && n_eff - sh.l > ctx->n) return KZG_ERR_DEGREE_TOO_HIGH;
    } else {
        rc = copy_unlocked(ctx, lk, s0.stream, s0.cpoly.dev(), coeffs, n_eff * 32, hipMemcpyHostToDevice, "hipMemcpyAsync (cells)");
        if (rc) return rc;
    }
    if (out_cells && n_eff < sh.N)
        HIP_TRY(ctx, hipMemsetAsync(s0.cpoly.dev() + 8 * n_eff, 0, (sh.N - n_eff) * 32, s0.stream));
    return cells_run(ctx, lk, slot0, sh, n_eff, out_cells, out_proofs);
}
// a multi-device context: a replicated SRS forwards to one device; a range-split one holds no device with the whole SRS
static kzg_ctx* cells_kid(kzg_ctx* ctx, int* rc) {
    if (multi_mode(ctx->multi) != kMultiReplicate) {
        ctx->last_error = "cells: a range-split multi-device context cannot prove cells (replicate the SRS instead)";
        *rc = KZG_ERR_INVALID_ARG;
        return nullptr;
    }
    return multi_kid(ctx->multi, 0);
}

int kzg_cells_and_proofs(kzg_ctx* ctx, const uint64_t* coeffs, size_t n, unsigned log_domain, unsigned log_cell,
                         uint64_t* out_cells, uint64_t* out_proofs) {
    CellsShape sh;
    if (!ctx || !out_proofs || (!coeffs && n) || !cells_shape(n, log_domain, log_cell, &sh)) return KZG_ERR_INVALID_ARG;
    if (ctx->multi) {
        int rc = KZG_OK;
        kzg_ctx* kid = cells_kid(ctx, &rc);
        return kid ? kzg_cells_and_proofs(kid, coeffs, n, log_domain, log_cell, out_cells, out_proofs) : rc;
    }
    return cells_host(ctx, coeffs, n ? cells_trim(coeffs, n) : 0, nullptr, 0, sh, out_cells, out_proofs);
}

int kzg_cells_and_proofs_evaluations(kzg_ctx* ctx, const uint64_t* evals, size_t n, unsigned log_domain, unsigned log_cell,
                                     uint64_t* out_cells, uint64_t* out_proofs) {
    CellsShape sh;
    uint32_t lg = 0;
    if (!ctx || !evals || !out_proofs || !ntt_log(n, &lg) || !cells_shape(n, log_domain, log_cell, &sh)) return KZG_ERR_INVALID_ARG;
    if (ctx->multi) {
        int rc = KZG_OK;
        kzg_ctx* kid = cells_kid(ctx, &rc);
        return kid ? kzg_cells_and_proofs_evaluations(kid, evals, n, log_domain, log_cell, out_cells, out_proofs) : rc;
    }
    return cells_host(ctx, nullptr, 0, evals, n, sh, out_cells, out_proofs);
}

int kzg_quotient_cells(kzg_ctx* ctx, const uint64_t* coeffs, size_t n, unsigned log_domain, unsigned log_cell, size_t first_cell,
                       size_t count, uint64_t* out_q, size_t* out_qn) {
    CellsShape sh;
    if (!ctx || !out_qn || (!coeffs && n) || !cells_shape(n, log_domain, log_cell, &sh)) return KZG_ERR_INVALID_ARG;
    if (first_cell > sh.cells || count > sh.cells - first_cell || (!out_q && n > sh.l && count)) return KZG_ERR_INVALID_ARG;
    if (ctx->multi) return kzg_quotient_cells(multi_kid(ctx->multi, 0), coeffs, n, log_domain, log_cell, first_cell, count, out_q, out_qn);
    const size_t n_eff = n ? cells_trim(coeffs, n) : 0;
    const size_t nq = n_eff > sh.l ? n_eff - sh.l : 0;
    *out_qn = 0;
    if (n > sh.l && count) std::memset(out_q, 0, count * (n - sh.l) * 32);
    if (!nq || !count) {
        *out_qn = nq;
        return KZG_OK;
    }
    std::unique_lock<std::mutex> lk(ctx->mu);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    int rc = ensure_ntt(ctx);
    if (rc) return rc;
    const int slot = reserve_slot(ctx, lk, true);
    if (slot < 0) return KZG_ERR_BUSY;
    SlotLease lease{ctx, slot};
    Slot& s = ctx->slots[slot];
    rc = ensure_slot_basics(ctx, s);  // needs no SRS
    if (rc == KZG_OK) rc = ensure_cells_poly(ctx, s, n_eff);
    if (rc == KZG_OK) rc = ensure_poly(ctx, s, count * nq);
    if (rc == KZG_OK) rc = s.cagg.reserve(ctx, cells_agg_words((uint32_t)nq, sh.log_l, (uint32_t)count) * 4, s.stream);
    if (rc) return rc;
    HIP_TRY(ctx, hipMemcpyAsync(s.cpoly.dev(), coeffs, n_eff * 32, hipMemcpyHostToDevice, s.stream));
    launch_cell_quotients(s.stream, s.cpoly.dev(), (uint32_t)nq, sh.log_n, sh.log_l, (uint32_t)first_cell, (uint32_t)count,
                          ctx->ntt_tw.p, s.cagg.dev(), s.q.dev(), nq);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipMemcpy2DAsync(out_q, (n - sh.l) * 32, s.q.dev(), nq * 32, nq * 32, count, hipMemcpyDeviceToHost, s.stream));
    HIP_TRY(ctx, hipStreamSynchronize(s.stream));
    *out_qn = nq;
    return KZG_OK;
}

// ---- FK20: every cell proof of a batch of polynomials through G1 DFTs (fk20_kernels.hip) ----------
// The call holds the context's mutex and one slot (for its stream and the cells' NTT buffers) for its whole length: other
// calls on the context wait for it, and an SRS replacement waits for the slot like for any other call.
namespace {
// lambda = z^2 - 1, z = -0xd201000000010000: [lambda](x, y) = (beta x, y) on G1 (fk20_kernels.hip), r = lambda^2 + lambda + 1
const unsigned __int128 kGlvLambda = ((unsigned __int128)0xac45a4010001a402ULL << 64) | 0x00000000ffffffffULL;
// w (blst_fr, Montgomery) = k1 + k2 lambda with k1 = w mod lambda, k2 = w div lambda: both below 2^128 since w < r
Glv glv_split(const hf::Fr& mont) {
    const hf::Fr one_raw = {{1, 0, 0, 0}};
    const hf::Fr v = hf::fr_mul(mont, one_raw);  // the plain integer
    unsigned __int128 rem = 0, q = 0;
    for (int bit = 255; bit >= 0; bit--) {
        const bool over = (uint64_t)(rem >> 127) != 0;  // rem << 1 leaves 128 bits: it is above lambda then
        rem = (rem << 1) | ((v.l[bit >> 6] >> (bit & 63)) & 1);
        q <<= 1;
        if (over || rem >= kGlvLambda) {
            rem -= kGlvLambda;
            q |= 1;
        }
    }
    Glv g;
    g.k1[0] = (uint64_t)rem;
    g.k1[1] = (uint64_t)(rem >> 64);
    g.k2[0] = (uint64_t)q;
    g.k2[1] = (uint64_t)(q >> 64);
    return g;
}
hf::Fr fr_pow2(uint32_t lg) {
    hf::Fr v = hf::kFrOne;
    for (uint32_t i = 0; i < lg; i++) v = hf::fr_add(v, v);
    return v;
}
enum : int { kWsCoef = 0, kWsScalA, kWsScalB, kWsPart, kWsX1, kWsX2, kWsX3, kWsAff, kWsPrefix, kWsP1, kWsCount };
constexpr size_t kFk20MaxBatch = 64;              // polynomials per pass through the workspaces, at most
constexpr size_t kFk20WsBudget = (size_t)4 << 30;  // ... and fewer when their workspaces would pass this
constexpr uint32_t kFk20CombChunk = 8192;         // bases per comb-table launch (XYZZ temporaries: 1 GiB) and per streamed chunk
uint32_t log2_ceil(size_t v) {
    uint32_t k = 0;
    while (((size_t)1 << k) < v) k++;
    return k;
}
// what the comb tables of all l L bases may occupy to be kept: KZG_FK20_TABLE_MB, else a quarter of the free memory up to
// 16 GiB.  Above it the tables are built per call, a chunk of positions at a time, and freed again.
size_t fk20_table_budget() {
    if (const char* v = std::getenv("KZG_FK20_TABLE_MB")) return (size_t)std::strtoull(v, nullptr, 10) << 20;
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) free_b = 0;
    const size_t cap = (size_t)16 << 30;
    return free_b / 4 < cap ? free_b / 4 : cap;
}
}  // namespace

// the split twiddles w_(2^lg)^e, e < 2^lg, for every transform of at most 2^lg points (device current)
static int ensure_glv(kzg_ctx* ctx, std::unique_lock<std::mutex>& lk, uint32_t lg, hipStream_t st) {
    if (lg < 1) lg = 1;
    if (ctx->glv.p && ctx->glv_log >= lg) return KZG_OK;
    const size_t len = (size_t)1 << lg;
    std::vector<Glv> h(len);
    const hf::Fr w = hf::fr_domain_root(lg);
    hf::Fr v = hf::kFrOne;
    for (size_t e = 0; e < len; e++) {
        h[e] = glv_split(v);
        v = hf::fr_mul(v, w);
    }
    int rc = sync_unlocked(ctx, lk, st, "fk20");  // nothing in flight reads the old table
    if (rc) return rc;
    ctx->glv.reset();
    rc = ctx->glv.reserve(ctx, len * sizeof(Glv));
    if (rc) return rc;
    ctx->glv_log = lg;
    HIP_TRY(ctx, hipMemcpyAsync(ctx->glv.p, h.data(), len * sizeof(Glv), hipMemcpyHostToDevice, st));
    return sync_unlocked(ctx, lk, st, "fk20");  // h goes out of scope
}
// comb tables of bases [first, first + count) ((i, r) order) into dst, through tmp / prefix (kFk20CombChunk bases each)
static void enqueue_comb(kzg_ctx* ctx, hipStream_t st, uint32_t log_L, uint32_t log_l, uint64_t first, uint64_t count,
                         void* dst, void* tmp, void* prefix) {
    for (uint64_t f = 0; f < count; f += kFk20CombChunk) {
        const uint32_t c = (uint32_t)(count - f < kFk20CombChunk ? count - f : kFk20CombChunk);
        launch_fk20_comb(st, ctx->fk20_B.p, log_L, log_l, first + f, c, tmp);
        launch_xyzz_to_affine(st, tmp, c * kFk20CombEntries, (char*)dst + f * kFk20CombEntries * kAffineBytes, prefix);
    }
}
// the SRS side of (L, l): B_r = DFT_L(S_r), r < l, and their comb tables when they fit fk20_table_budget()
static int ensure_fk20_table(kzg_ctx* ctx, std::unique_lock<std::mutex>& lk, hipStream_t st, uint32_t log_L, uint32_t log_l) {
    if (ctx->fk20_B.p && ctx->fk20_log_L == log_L && ctx->fk20_log_l == log_l) return KZG_OK;
    int rc = sync_unlocked(ctx, lk, st, "fk20");
    if (rc) return rc;
    ctx->fk20_B.reset();
    ctx->fk20_tab.reset();
    const size_t bases = (size_t)1 << (log_L + log_l);
    const size_t tab_bytes = bases * kFk20CombEntries * kAffineBytes;
    DevBuf S, B1, B2;
    HIP_TRY(ctx, hipMalloc(&S.p, bases * kXyzzBytes));
    HIP_TRY(ctx, hipMalloc(&B1.p, bases * kXyzzBytes));
    HIP_TRY(ctx, hipMalloc(&B2.p, bases * kXyzzBytes));
    launch_fk20_srs_gather(st, ctx->table.p, ctx->n, log_L, log_l, S.p);
    const void* B = launch_g1_dft(st, S.p, B1.p, B2.p, log_L, (uint64_t)1 << log_l, (const Glv*)ctx->glv.p, ctx->glv_log, false);
    std::swap(ctx->fk20_B.p, B == B1.p ? B1.p : B2.p);  // kept
    ctx->fk20_log_L = log_L;
    ctx->fk20_log_l = log_l;
    if (tab_bytes <= fk20_table_budget()) {
        DevBuf tab;
        if (hipMalloc(&tab.p, tab_bytes) == hipSuccess) {
            DevBuf tmp, prefix;
            const size_t chunk = bases < kFk20CombChunk ? bases : kFk20CombChunk;
            HIP_TRY(ctx, hipMalloc(&tmp.p, chunk * kFk20CombEntries * kXyzzBytes));
            HIP_TRY(ctx, hipMalloc(&prefix.p, chunk * kFk20CombEntries * 64));
            std::swap(ctx->fk20_tab.p, tab.p);
            enqueue_comb(ctx, st, log_L, log_l, 0, bases, ctx->fk20_tab.p, tmp.p, prefix.p);
            HIP_TRY(ctx, hipGetLastError());
            return sync_unlocked(ctx, lk, st, "fk20");  // before the temporaries go
        }
        (void)hipGetLastError();  // no room after all: the tables are streamed per call
    }
    HIP_TRY(ctx, hipGetLastError());
    return sync_unlocked(ctx, lk, st, "fk20");
}
// shape of the Toeplitz step for polynomials of at most n' coefficients (n' > l): m = ceil(n' / l), L = 2^log_L >= 2m
static bool fk20_shape(kzg_ctx* ctx, size_t n_max, uint32_t log_l, uint32_t* m, uint32_t* log_L) {
    const size_t mm = (n_max + ((size_t)1 << log_l) - 1) >> log_l;
    *m = (uint32_t)mm;
    *log_L = log2_ceil(2 * mm);
    if (*log_L > kNttMaxLog) {
        ctx->last_error = "fk20: the circulant of this shape would exceed 2^22 points (l = 1 with n' > 2^21)";
        return false;
    }
    // any L >= 2m works: a cached transform of the same l up to twice as long serves instead of being rebuilt
    if (ctx->fk20_B.p && ctx->fk20_log_l == log_l && ctx->fk20_log_L >= *log_L && ctx->fk20_log_L <= *log_L + 1)
        *log_L = ctx->fk20_log_L;
    return true;
}
// positions per streamed chunk when the comb tables are not kept
static uint32_t fk20_stream_positions(uint32_t log_L, uint32_t log_l) {
    const uint32_t ci = kFk20CombChunk >> log_l;
    return ci < (1u << log_L) ? ci : (1u << log_L);
}

// `batch` polynomials (coefficients at c, n_max per polynomial, contiguous) -> proofs (batch x 2^log_M blst_p1).  d_src: the
// coefficients are in device memory there (same stride) and coeffs is not read.  keep_affine: the normalised affine proofs stay
// in the kWsAff workspace, enqueued on st and not waited for, and out_proofs is not written.
static int fk20_proofs(kzg_ctx* ctx, std::unique_lock<std::mutex>& lk, hipStream_t st, const uint64_t* coeffs, size_t stride,
                       size_t batch, size_t n_max, uint32_t m, uint32_t log_L, uint32_t log_l, uint32_t log_M,
                       uint64_t* out_proofs, void* stream_tab, void* stream_tmp, void* stream_prefix, const void* d_src = nullptr,
                       bool keep_affine = false) {
    const size_t L = (size_t)1 << log_L, l = (size_t)1 << log_l, M = (size_t)1 << log_M;
    const size_t X = L > M ? L : M;
    const bool kept = ctx->fk20_tab.p != nullptr;
    const uint32_t ci = kept ? (uint32_t)L : fk20_stream_positions(log_L, log_l);
    void *coef, *sa, *sb, *part, *x1, *x2, *x3, *aff, *prefix, *p1;
    int rc = ctx->fk20_ws.get(ctx, kWsCoef, batch * n_max * 32, &coef);
    if (rc == KZG_OK) rc = ctx->fk20_ws.get(ctx, kWsScalA, batch * l * L * 32, &sa);
    if (rc == KZG_OK) rc = ctx->fk20_ws.get(ctx, kWsScalB, batch * l * L * 32, &sb);
    if (rc == KZG_OK) rc = ctx->fk20_ws.get(ctx, kWsPart, l > 1 ? batch * l * ci * kXyzzBytes : 0, &part);
    if (rc == KZG_OK) rc = ctx->fk20_ws.get(ctx, kWsX1, batch * X * kXyzzBytes, &x1);
    if (rc == KZG_OK) rc = ctx->fk20_ws.get(ctx, kWsX2, batch * X * kXyzzBytes, &x2);
    if (rc == KZG_OK) rc = ctx->fk20_ws.get(ctx, kWsX3, batch * X * kXyzzBytes, &x3);
    if (rc == KZG_OK) rc = ctx->fk20_ws.get(ctx, kWsAff, batch * M * kAffineBytes, &aff);
    if (rc == KZG_OK) rc = ctx->fk20_ws.get(ctx, kWsPrefix, batch * M * 64, &prefix);
    if (rc == KZG_OK) rc = ctx->fk20_ws.get(ctx, kWsP1, batch * M * 144, &p1);
    if (rc) return rc;
    if (d_src) HIP_TRY(ctx, hipMemcpy2DAsync(coef, n_max * 32, d_src, stride * 32, n_max * 32, batch, hipMemcpyDeviceToDevice, st));
    else HIP_TRY(ctx, hipMemcpy2DAsync(coef, n_max * 32, coeffs, stride * 32, n_max * 32, batch, hipMemcpyHostToDevice, st));
    const Fr30 inv_L = fr30_arg_from_mont256(hf::fr_inv(fr_pow2(log_L)));
    const uint32_t* scal = launch_fk20_fr_side(st, (const uint32_t*)coef, (uint32_t)n_max, m, log_L, log_l, batch, ctx->ntt_tw.p,
                                               inv_L, (uint32_t*)sa, (uint32_t*)sb);
    if (kept) {
        launch_fk20_pointwise(st, scal, ctx->fk20_tab.p, log_L, log_l, 0, (uint32_t)L, batch, part, x1);
    } else {  // the comb tables of one chunk of positions at a time
        for (uint32_t i0 = 0; i0 < L; i0 += ci) {
            enqueue_comb(ctx, st, log_L, log_l, (uint64_t)i0 << log_l, (uint64_t)ci << log_l, stream_tab, stream_tmp, stream_prefix);
            launch_fk20_pointwise(st, scal, stream_tab, log_L, log_l, i0, ci, batch, part, x1);
        }
    }
    const Glv* tw = (const Glv*)ctx->glv.p;
    const void* conv = launch_g1_dft(st, x1, x2, x3, log_L, batch, tw, ctx->glv_log, true);  // 1/L went into the scalars
    // log_L >= 2: conv is x2 or x3; the second DFT ping-pongs through x1 and conv, free once the selection has read it
    void* h = conv == x2 ? x3 : x2;
    launch_fk20_select(st, conv, log_L, m, log_M, batch, h);
    const void* res = launch_g1_dft(st, h, x1, (void*)conv, log_M, batch, tw, ctx->glv_log, false);
    launch_xyzz_to_affine(st, res, (uint32_t)(batch * M), aff, prefix);
    if (keep_affine) {
        HIP_TRY(ctx, hipGetLastError());
        return KZG_OK;
    }
    launch_affine_to_p1(st, aff, (uint32_t)(batch * M), p1);
    HIP_TRY(ctx, hipGetLastError());
    rc = sync_unlocked(ctx, lk, st, "fk20");
    if (rc) return rc;
    HIP_TRY(ctx, hipMemcpyAsync(out_proofs, p1, batch * M * 144, hipMemcpyDeviceToHost, st));
    return sync_unlocked(ctx, lk, st, "fk20");
}

static int fk20_host(kzg_ctx* ctx, const uint64_t* coeffs, size_t n, size_t batch, size_t stride, const CellsShape& sh,
                     uint64_t* out_cells, uint64_t* out_proofs) {
    std::lock_guard<std::mutex> lkf(ctx->fk20_mu);
    std::unique_lock<std::mutex> lk(ctx->mu);
    if (!ctx->n || !ctx->slots_ready) return KZG_ERR_NO_SRS;
    std::vector<size_t> neff(batch);
    size_t n_max = 0;
    for (size_t b = 0; b < batch; b++) {
        neff[b] = n ? cells_trim(coeffs + 4 * b * stride, n) : 0;
        if (neff[b] > sh.l && neff[b] - sh.l > ctx->n) {
            ctx->last_error = "fk20: polynomial " + std::to_string(b) + ": n' - l = " + std::to_string(neff[b] - sh.l) +
                              " exceeds the SRS (" + std::to_string(ctx->n) + " points)";
            return KZG_ERR_DEGREE_TOO_HIGH;
        }
        if (neff[b] > n_max) n_max = neff[b];
    }
    uint32_t m = 0, log_L = 0;
    if (n_max > sh.l && !fk20_shape(ctx, n_max, sh.log_l, &m, &log_L)) return KZG_ERR_INVALID_ARG;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    int rc = ensure_ntt(ctx);
    if (rc) return rc;
    const int slot0 = reserve_slot(ctx, lk, true);
    if (slot0 < 0) return KZG_ERR_BUSY;
    SlotLease lease{ctx, slot0};
    Slot& s0 = ctx->slots[slot0];
    if (out_cells) {  // per polynomial: forward NTT of P padded to N, gathered into cell-major order (as kzg_cells_and_proofs)
        rc = ensure_cells_poly(ctx, s0, sh.N);
        if (rc == KZG_OK) rc = ensure_poly(ctx, s0, sh.N);
        if (rc) return rc;
        for (size_t b = 0; b < batch; b++) {
            if (neff[b]) HIP_TRY(ctx, hipMemcpyAsync(s0.cpoly.dev(), coeffs + 4 * b * stride, neff[b] * 32, hipMemcpyHostToDevice, s0.stream));
            if (neff[b] < sh.N) HIP_TRY(ctx, hipMemsetAsync(s0.cpoly.dev() + 8 * neff[b], 0, (sh.N - neff[b]) * 32, s0.stream));
            rc = ntt_into_stage(ctx, s0, s0.cpoly.dev(), sh.log_n, false);
            if (rc) return rc;
            launch_cells_gather(s0.stream, s0.stage.dev(), s0.q.dev(), sh.log_n, sh.log_l);
            HIP_TRY(ctx, hipGetLastError());
            rc = sync_unlocked(ctx, lk, s0.stream, "fk20");
            if (rc) return rc;
            HIP_TRY(ctx, hipMemcpyAsync(out_cells + 4 * sh.N * b, s0.q.dev(), sh.N * 32, hipMemcpyDeviceToHost, s0.stream));
            rc = sync_unlocked(ctx, lk, s0.stream, "fk20");
            if (rc) return rc;
        }
    }
    if (n_max <= sh.l) {  // every polynomial is its own interpolant on every cell
        const hf::P1 inf = hf::p1_inf();
        for (size_t j = 0; j < batch * sh.cells; j++) write_p1(out_proofs + 18 * j, inf);
        return KZG_OK;
    }
    const uint32_t log_M = sh.log_n - sh.log_l;
    rc = ensure_glv(ctx, lk, log_L > log_M ? log_L : log_M, s0.stream);
    if (rc == KZG_OK) rc = ensure_fk20_table(ctx, lk, s0.stream, log_L, sh.log_l);
    if (rc) return rc;
    // polynomials per pass: at most kFk20MaxBatch, fewer when their workspaces would pass kFk20WsBudget
    const size_t L = (size_t)1 << log_L, M = (size_t)1 << log_M, X = L > M ? L : M;
    const bool kept = ctx->fk20_tab.p != nullptr;
    const size_t ci = kept ? L : fk20_stream_positions(log_L, sh.log_l);
    const size_t per_poly = n_max * 32 + sh.l * L * 64 + (sh.l > 1 ? sh.l * ci * kXyzzBytes : 0) + 3 * X * kXyzzBytes + M * 336;
    size_t chunk = kFk20WsBudget / per_poly;
    chunk = chunk < 1 ? 1 : (chunk > kFk20MaxBatch ? kFk20MaxBatch : chunk);
    DevBuf stab, stmp, spre;  // the streamed comb tables of one chunk of positions, freed with the call
    if (!kept) {
        const size_t sb = ci << sh.log_l;
        HIP_TRY(ctx, hipMalloc(&stab.p, sb * kFk20CombEntries * kAffineBytes));
        HIP_TRY(ctx, hipMalloc(&stmp.p, sb * kFk20CombEntries * kXyzzBytes));
        HIP_TRY(ctx, hipMalloc(&spre.p, sb * kFk20CombEntries * 64));
    }
    for (size_t b0 = 0; b0 < batch && rc == KZG_OK; b0 += chunk) {
        const size_t bc = batch - b0 < chunk ? batch - b0 : chunk;
        rc = fk20_proofs(ctx, lk, s0.stream, coeffs + 4 * b0 * stride, stride, bc, n_max, m, log_L, sh.log_l, log_M,
                         out_proofs + 18 * sh.cells * b0, stab.p, stmp.p, spre.p);
    }
    if (!kept) {  // the DevBufs free when the call returns; nothing in flight may still read them
        const int r2 = sync_unlocked(ctx, lk, s0.stream, "fk20");
        if (rc == KZG_OK) rc = r2;
    }
    return rc;
}

int kzg_cells_and_proofs_fk20(kzg_ctx* ctx, const uint64_t* coeffs, size_t n, size_t batch, size_t stride_coeffs,
                              unsigned log_domain, unsigned log_cell, uint64_t* out_cells, uint64_t* out_proofs) {
    CellsShape sh;
    if (!ctx || (!out_proofs && batch) || (!coeffs && n && batch) || !cells_shape(n, log_domain, log_cell, &sh))
        return KZG_ERR_INVALID_ARG;
    if (batch > 1 && stride_coeffs < n) {
        ctx->last_error = "fk20: stride_coeffs is below n";
        return KZG_ERR_INVALID_ARG;
    }
    if (ctx->multi) {
        int rc = KZG_OK;
        kzg_ctx* kid = cells_kid(ctx, &rc);
        return kid ? kzg_cells_and_proofs_fk20(kid, coeffs, n, batch, stride_coeffs, log_domain, log_cell, out_cells, out_proofs) : rc;
    }
    if (!batch) return KZG_OK;
    return fk20_host(ctx, coeffs, n, batch, batch > 1 ? stride_coeffs : n, sh, out_cells, out_proofs);
}

int kzg_fk20_prepare(kzg_ctx* ctx, size_t n, unsigned log_cell) {
    if (!ctx || log_cell > KZG_MAX_CELL_LOG) return KZG_ERR_INVALID_ARG;
    if (ctx->multi) {
        int rc = KZG_OK;
        kzg_ctx* kid = cells_kid(ctx, &rc);
        return kid ? kzg_fk20_prepare(kid, n, log_cell) : rc;
    }
    std::lock_guard<std::mutex> lkf(ctx->fk20_mu);
    std::unique_lock<std::mutex> lk(ctx->mu);
    if (!ctx->n || !ctx->slots_ready) return KZG_ERR_NO_SRS;
    if (n <= ((size_t)1 << log_cell)) return KZG_OK;  // such polynomials have infinity proofs: nothing to build
    uint32_t m = 0, log_L = 0;
    if (!fk20_shape(ctx, n, log_cell, &m, &log_L)) return KZG_ERR_INVALID_ARG;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const int slot = reserve_slot(ctx, lk, true);
    if (slot < 0) return KZG_ERR_BUSY;
    SlotLease lease{ctx, slot};
    Slot& s = ctx->slots[slot];
    int rc = ensure_glv(ctx, lk, log_L, s.stream);
    if (rc == KZG_OK) rc = ensure_fk20_table(ctx, lk, s.stream, log_L, log_cell);
    return rc;
}

int kzg_g1_dft(kzg_ctx* ctx, const uint64_t* in_p1, size_t m, int inverse, uint64_t* out_p1) {
    uint32_t lg = 0;
    if (!ctx || !in_p1 || !out_p1 || !ntt_log(m, &lg)) return KZG_ERR_INVALID_ARG;
    if (ctx->multi) return kzg_g1_dft(multi_kid(ctx->multi, 0), in_p1, m, inverse, out_p1);  // needs no SRS
    std::lock_guard<std::mutex> lkf(ctx->fk20_mu);
    std::unique_lock<std::mutex> lk(ctx->mu);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const int slot = reserve_slot(ctx, lk, true);
    if (slot < 0) return KZG_ERR_BUSY;
    SlotLease lease{ctx, slot};
    Slot& s = ctx->slots[slot];
    int rc = ensure_slot_basics(ctx, s);  // needs no SRS
    if (rc == KZG_OK) rc = ensure_glv(ctx, lk, lg, s.stream);
    void *jac, *aff, *prefix, *x1, *x2, *x3;
    if (rc == KZG_OK) rc = ctx->fk20_ws.get(ctx, kWsP1, m * 144, &jac);
    if (rc == KZG_OK) rc = ctx->fk20_ws.get(ctx, kWsAff, m * kAffineBytes, &aff);
    if (rc == KZG_OK) rc = ctx->fk20_ws.get(ctx, kWsPrefix, m * 64, &prefix);
    if (rc == KZG_OK) rc = ctx->fk20_ws.get(ctx, kWsX1, m * kXyzzBytes, &x1);
    if (rc == KZG_OK) rc = ctx->fk20_ws.get(ctx, kWsX2, m * kXyzzBytes, &x2);
    if (rc == KZG_OK) rc = ctx->fk20_ws.get(ctx, kWsX3, m * kXyzzBytes, &x3);
    if (rc) return rc;
    HIP_TRY(ctx, hipMemcpyAsync(jac, in_p1, m * 144, hipMemcpyHostToDevice, s.stream));
    launch_jacobian_to_affine(s.stream, jac, (uint32_t)m, aff, prefix);
    launch_affine_to_xyzz(s.stream, aff, m, x1);
    void* res = (void*)launch_g1_dft(s.stream, x1, x2, x3, lg, 1, (const Glv*)ctx->glv.p, ctx->glv_log, inverse != 0);
    if (inverse) launch_g1_scale(s.stream, res, m, glv_split(hf::fr_inv(fr_pow2(lg))));
    launch_xyzz_to_affine(s.stream, res, (uint32_t)m, aff, prefix);
    launch_affine_to_p1(s.stream, aff, (uint32_t)m, jac);
    HIP_TRY(ctx, hipGetLastError());
    rc = sync_unlocked(ctx, lk, s.stream, "fk20");
    if (rc) return rc;
    HIP_TRY(ctx, hipMemcpyAsync(out_p1, jac, m * 144, hipMemcpyDeviceToHost, s.stream));
    return sync_unlocked(ctx, lk, s.stream, "fk20");
}

// ---- the Lagrange basis and the calls on values over it (lagrange_kernels.hip) -----------------------
// L_i = [l_i(s)] G1 = (1/n) sum_j w^(-ij) SRS[j]: an inverse G1 DFT of SRS[0 .. n), normalised into level 0 of a window table
// of its own.  Locks: fk20_mu (the split twiddles), then ctx->mu; the build waits for the device without ctx->mu.

static int forwarded(kzg_ctx* ctx, kzg_ctx* kid, int rc);  // (below: a kid's status with its error text)
// the lg-bit reversal of i
static uint32_t lagrange_brp(uint32_t i, uint32_t lg) {
    uint32_t r = 0;
    for (uint32_t b = 0; b < lg; b++) r |= ((i >> b) & 1u) << (lg - 1 - b);
    return r;
}
// levels 1 .. W-1 of a basis table whose level 0 (n records) is in tab; d_xyzz_tmp: n XYZZ records, d_prefix: n x 64 bytes
static void lagrange_enqueue_levels(kzg_ctx* ctx, hipStream_t st, void* tab, size_t n, void* d_xyzz_tmp, void* d_prefix) {
    for (uint32_t j = 1; j < ctx->cfg.W; j++)
        launch_table_window(st, (char*)tab + (size_t)(j - 1) * n * kAffineBytes, (uint32_t)n, ctx->cfg.level_bits, d_xyzz_tmp, d_prefix,
                            (char*)tab + (size_t)j * n * kAffineBytes);
}
// The finished table becomes the context's basis (fk20_mu and ctx->mu held, the caller holds no slot).  No synchronous call is
// between its steps and nothing in flight reads the basis that goes: from the quiesce on ctx->mu is not released, so no job can
// start on it, and the ones that did have ended.  gen: ctx->srs_gen when the table was started.
static int lagrange_adopt(kzg_ctx* ctx, std::unique_lock<std::mutex>& lk, DevBuf& tab, size_t n, uint64_t gen) {
    quiesce(ctx, lk);
    if (gen != ctx->srs_gen || !ctx->n || !ctx->slots_ready) {
        ctx->last_error = "lagrange basis: the SRS was replaced while the basis was built";
        return KZG_ERR_NO_SRS;
    }
    ctx->lag_n = 0;
    if (ctx->lag_table.p) {
        int rc = drain_all(ctx);
        if (rc) return rc;
        ctx->lag_table.reset();
    }
    std::swap(ctx->lag_table.p, tab.p);
    std::swap(ctx->lag_table.cap, tab.cap);
    ctx->lag_n = n;
    return KZG_OK;
}
// builds the basis of 2^lg points, replacing a held one (fk20_mu and ctx->mu held; device current).  The held basis stays in
// use while the new one is built.
static int lagrange_build(kzg_ctx* ctx, std::unique_lock<std::mutex>& lk, uint32_t lg) {
    const size_t n = (size_t)1 << lg;
    if (!ctx->n || !ctx->slots_ready) return KZG_ERR_NO_SRS;
    if (n > ctx->n) return KZG_ERR_DEGREE_TOO_HIGH;
    if (ctx->lag_table.p && ctx->lag_n == n) return KZG_OK;
    DevBuf tab;
    const uint64_t gen = ctx->srs_gen;
    {
        const int slot = reserve_slot(ctx, lk, true);  // (keeps an SRS replacement out while ctx->mu is released below)
        if (slot < 0) return KZG_ERR_BUSY;
        SlotLease lease{ctx, slot};
        hipStream_t st = ctx->slots[slot].stream;
        int rc = ensure_glv(ctx, lk, lg, st);
        if (rc) return rc;
        DevBuf x1, x2, x3, prefix;
        rc = tab.reserve(ctx, (size_t)ctx->cfg.W * n * kAffineBytes);
        if (rc == KZG_OK) rc = x1.reserve(ctx, n * kXyzzBytes);
        if (rc == KZG_OK) rc = x2.reserve(ctx, n * kXyzzBytes);
        if (rc == KZG_OK) rc = x3.reserve(ctx, n * kXyzzBytes);
        if (rc == KZG_OK) rc = prefix.reserve(ctx, n * 64);
        if (rc) return rc;
        launch_affine_to_xyzz(st, ctx->table.p, n, x1.p);
        void* res = (void*)launch_g1_dft(st, x1.p, x2.p, x3.p, lg, 1, (const Glv*)ctx->glv.p, ctx->glv_log, true);
        launch_g1_scale(st, res, n, glv_split(hf::fr_inv(fr_pow2(lg))));
        launch_xyzz_to_affine(st, res, (uint32_t)n, tab.p, prefix.p);
        lagrange_enqueue_levels(ctx, st, tab.p, n, res == x1.p ? x2.p : x1.p /* (the transform is in level 0 now) */, prefix.p);
        HIP_TRY(ctx, hipGetLastError());
        rc = sync_unlocked(ctx, lk, st, "lagrange basis");  // before the temporaries go
        if (rc) return rc;
    }
    return lagrange_adopt(ctx, lk, tab, n, gen);
}
// a multi-device context: a replicated SRS forwards to the device the evaluation calls forward to, a range-split one holds
// no whole SRS to transform
static kzg_ctx* lagrange_kid(kzg_ctx* ctx, int* rc) {
    if (multi_mode(ctx->multi) != kMultiReplicate) {
        ctx->last_error = "the Lagrange basis needs the whole SRS on one device: not on a range-split multi-device context";
        *rc = KZG_ERR_INVALID_ARG;
        return nullptr;
    }
    if (!multi_srs_len(ctx->multi)) {
        *rc = KZG_ERR_NO_SRS;
        return nullptr;
    }
    return multi_kid(ctx->multi, 0);
}
// the basis of n points is held when this returns KZG_OK with ctx->mu (lk) held: built now unless it was there
static int lagrange_ensure(kzg_ctx* ctx, std::unique_lock<std::mutex>& lk, size_t n, uint32_t lg) {
    if (!ctx->n || !ctx->slots_ready) return KZG_ERR_NO_SRS;
    if (n > ctx->n) return KZG_ERR_DEGREE_TOO_HIGH;
    if (ctx->lag_table.p && ctx->lag_n == n) return KZG_OK;
    lk.unlock();  // fk20_mu is taken before ctx->mu
    std::lock_guard<std::mutex> lkf(ctx->fk20_mu);
    lk.lock();
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    return lagrange_build(ctx, lk, lg);
}

int kzg_lagrange_prepare(kzg_ctx* ctx, unsigned log_n) {
    if (!ctx || log_n > KZG_NTT_MAX_LOG) return KZG_ERR_INVALID_ARG;
    if (ctx->multi) {
        int rc = KZG_OK;
        kzg_ctx* kid = lagrange_kid(ctx, &rc);
        return kid ? forwarded(ctx, kid, kzg_lagrange_prepare(kid, log_n)) : rc;
    }
    std::lock_guard<std::mutex> lkf(ctx->fk20_mu);
    std::unique_lock<std::mutex> lk(ctx->mu);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    return lagrange_build(ctx, lk, log_n);
}

size_t kzg_lagrange_len(const kzg_ctx* ctx) {
    if (!ctx) return 0;
    if (ctx->multi) return multi_mode(ctx->multi) == kMultiReplicate ? kzg_lagrange_len(multi_kid(ctx->multi, 0)) : 0;
    std::lock_guard<std::mutex> lk(const_cast<kzg_ctx*>(ctx)->mu);
    return ctx->lag_table.p ? ctx->lag_n : 0;
}

int kzg_lagrange_read_g1(kzg_ctx* ctx, size_t index, size_t count, uint64_t* out_p1) {
    if (!ctx || !out_p1) return KZG_ERR_INVALID_ARG;
    if (ctx->multi) {
        int rc = KZG_OK;
        kzg_ctx* kid = lagrange_kid(ctx, &rc);
        return kid ? forwarded(ctx, kid, kzg_lagrange_read_g1(kid, index, count, out_p1)) : rc;
    }
    std::unique_lock<std::mutex> lk(ctx->mu);
    if (!ctx->lag_table.p || !ctx->lag_n) return KZG_ERR_NO_SRS;
    if (index > ctx->lag_n || count > ctx->lag_n - index) return KZG_ERR_INVALID_ARG;
    if (!count) return KZG_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    DevBuf d_p1;
    int rc = d_p1.reserve(ctx, count * 144);
    if (rc) return rc;
    hipStream_t st = ctx->slots[0].stream;
    launch_affine_to_p1(st, (const char*)ctx->lag_table.p + index * kAffineBytes, (uint32_t)count, d_p1.p);
    HIP_TRY(ctx, hipMemcpyAsync(out_p1, d_p1.p, count * 144, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    return KZG_OK;
}

int kzg_commit_lagrange_submit(kzg_ctx* ctx, int slot, const void* d_evals, size_t n) {
    KZG_SINGLE_DEVICE_ONLY(ctx);
    uint32_t lg = 0;
    if (!ctx || !d_evals || !ntt_log(n, &lg)) return KZG_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(ctx->mu);
    if (!ctx->n || !ctx->slots_ready) return KZG_ERR_NO_SRS;
    if (n > ctx->n) return KZG_ERR_DEGREE_TOO_HIGH;
    MsmBasis basis{};
    if (!lagrange_basis(ctx, n, &basis)) return KZG_ERR_NO_SRS;  // never builds
    return submit_commit_locked(ctx, slot, (const uint32_t*)d_evals, 1, n, true, false, &basis);
}

int kzg_commit_lagrange(kzg_ctx* ctx, const uint64_t* evals, size_t n, uint64_t out_p1[18]) {
    uint32_t lg = 0;
    if (!ctx || !evals || !out_p1 || !ntt_log(n, &lg)) return KZG_ERR_INVALID_ARG;
    if (ctx->multi) {
        int rc = KZG_OK;
        kzg_ctx* kid = lagrange_kid(ctx, &rc);
        return kid ? forwarded(ctx, kid, kzg_commit_lagrange(kid, evals, n, out_p1)) : rc;
    }
    std::unique_lock<std::mutex> lk(ctx->mu);
    int rc = lagrange_ensure(ctx, lk, n, lg);
    if (rc) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const int slot = reserve_slot(ctx, lk, true);
    if (slot < 0) return KZG_ERR_BUSY;
    SlotLease lease{ctx, slot};  // (a basis is replaced only when no synchronous call holds a slot: it stays until the submit)
    Slot& s = ctx->slots[slot];
    rc = ensure_poly(ctx, s, n);
    if (rc == KZG_OK) rc = upload_unlocked(ctx, lk, s, s.stage.dev(), evals, n * 32);
    MsmBasis basis{};
    if (rc == KZG_OK && !lagrange_basis(ctx, n, &basis)) rc = KZG_ERR_NO_SRS;
    if (rc == KZG_OK) rc = submit_commit_locked(ctx, slot, s.stage.dev(), 1, n, true, true, &basis);
    if (rc) return rc;
    await_unlocked(lk, s);
    return wait_locked(ctx, slot, out_p1);
}

int kzg_commit_lagrange_batch(kzg_ctx* ctx, const uint64_t* evals, size_t n, size_t batch, size_t stride, uint64_t* out_p1s) {
    uint32_t lg = 0;
    if (!ctx || (!evals && batch) || (!out_p1s && batch) || !ntt_log(n, &lg) || stride < n) return KZG_ERR_INVALID_ARG;
    if (ctx->multi) {
        int rc = KZG_OK;
        kzg_ctx* kid = lagrange_kid(ctx, &rc);
        return kid ? forwarded(ctx, kid, kzg_commit_lagrange_batch(kid, evals, n, batch, stride, out_p1s)) : rc;
    }
    {
        std::unique_lock<std::mutex> lk(ctx->mu);
        int rc = lagrange_ensure(ctx, lk, n, lg);
        if (rc) return rc;
    }
    // (a basis replaced between the two steps makes the batch answer KZG_ERR_NO_SRS, as a submit would)
    return commit_lagrange_batch_host(ctx, evals, n, stride, batch, out_p1s);
}

// the quotient on the values into s.q and the job's flag words (ctx->mu held, twiddles built, slot basics and buffers ready)
static int enqueue_lagrange_quotient(kzg_ctx* ctx, Slot& s, const uint32_t* d_evals, uint32_t lg, const uint64_t z[4],
                                     const uint64_t y[4]) {
    hf::Fr zf;
    std::memcpy(zf.l, z, 32);
    uint32_t yw[8];
    std::memcpy(yw, y, 32);
    std::memset(s.small.host(), 0, 64 * 4);  // (the slot's last job was collected: nothing in flight writes them)
    launch_lagrange_quotient(s.stream, d_evals, lg, fr30_arg_from_mont256(zf), fr30_from_limbs(yw),
                             fr30_arg_from_mont256(hf::fr_inv(fr_pow2(lg))), ctx->ntt_tw.p, s.q.dev(), s.lag_part.dev(), s.small.dev());
    HIP_TRY(ctx, hipGetLastError());
    return KZG_OK;
}
static int lagrange_slot_ready(kzg_ctx* ctx, Slot& s, size_t n, uint32_t lg) {
    int rc = ensure_ntt(ctx);
    if (rc == KZG_OK) rc = ntt_slot_ready(ctx, s, n);
    if (rc == KZG_OK) rc = s.lag_part.reserve(ctx, (size_t)lagrange_tiles(lg) * kLagPartialWords * 4);
    return rc;
}

// An opening from values on slot `slot`: the quotient on the values, then the MSM over the Lagrange table; wait_locked reads
// the flag words as it does for the coefficient route (constant polynomial, P(z) against y).
static int submit_open_lagrange_locked(kzg_ctx* ctx, int slot, const uint32_t* d_evals, size_t n, uint32_t lg, const uint64_t z[4],
                                       const uint64_t y[4], bool owned) {
    if (!ctx->n || !ctx->slots_ready) return KZG_ERR_NO_SRS;
    if (n > ctx->n) return KZG_ERR_DEGREE_TOO_HIGH;
    MsmBasis basis{};
    if (!lagrange_basis(ctx, n, &basis)) return KZG_ERR_NO_SRS;
    if (slot < 0 || slot >= kNumSlots) return KZG_ERR_INVALID_ARG;
    Slot& s = ctx->slots[slot];
    if (s.kind != (owned ? SLOT_RESERVED : SLOT_IDLE)) return KZG_ERR_BUSY;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    int rc = lagrange_slot_ready(ctx, s, n, lg);
    if (rc) return rc;
    s.timing = ctx->timing;
    s.end = s.stream;
    s.job_n = n;
    s.job_batch = 1;
    s.has_quotient = true;
    s.tail_checked = false;
    std::memcpy(s.open_y, y, 32);
    std::memset(&s.times, 0, sizeof s.times);
    if (s.timing) HIP_TRY(ctx, hipEventRecord(s.ev[6], s.stream));
    rc = enqueue_lagrange_quotient(ctx, s, d_evals, lg, z, y);
    if (rc) return rc;
    if (s.timing) HIP_TRY(ctx, hipEventRecord(s.ev[7], s.stream));
    rc = enqueue_msm(ctx, s, s.q.dev(), 1, n, 0, 1, 0, &basis);
    if (rc) return rc;
    HIP_TRY(ctx, hipEventRecord(s.done, s.end));
    s.kind = SLOT_OPEN;
    return KZG_OK;
}

int kzg_open_lagrange_submit(kzg_ctx* ctx, int slot, const void* d_evals, size_t n, const uint64_t z[4], const uint64_t y[4]) {
    KZG_SINGLE_DEVICE_ONLY(ctx);
    uint32_t lg = 0;
    if (!ctx || !d_evals || !z || !y || !ntt_log(n, &lg)) return KZG_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(ctx->mu);
    return submit_open_lagrange_locked(ctx, slot, (const uint32_t*)d_evals, n, lg, z, y, false);
}

int kzg_open_lagrange(kzg_ctx* ctx, const uint64_t* evals, size_t n, const uint64_t z[4], const uint64_t y[4], uint64_t out_p1[18]) {
    uint32_t lg = 0;
    if (!ctx || !evals || !z || !y || !out_p1 || !ntt_log(n, &lg)) return KZG_ERR_INVALID_ARG;
    if (ctx->multi) {
        int rc = KZG_OK;
        kzg_ctx* kid = lagrange_kid(ctx, &rc);
        return kid ? forwarded(ctx, kid, kzg_open_lagrange(kid, evals, n, z, y, out_p1)) : rc;
    }
    std::unique_lock<std::mutex> lk(ctx->mu);
    int rc = lagrange_ensure(ctx, lk, n, lg);
    if (rc) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const int slot = reserve_slot(ctx, lk, true);
    if (slot < 0) return KZG_ERR_BUSY;
    SlotLease lease{ctx, slot};
    Slot& s = ctx->slots[slot];
    rc = lagrange_slot_ready(ctx, s, n, lg);
    if (rc == KZG_OK) rc = upload_unlocked(ctx, lk, s, s.stage.dev(), evals, n * 32);
    if (rc == KZG_OK) rc = submit_open_lagrange_locked(ctx, slot, s.stage.dev(), n, lg, z, y, true);
    if (rc) return rc;
    await_unlocked(lk, s);
    return wait_locked(ctx, slot, out_p1);
}

int kzg_quotient_lagrange(kzg_ctx* ctx, const uint64_t* evals, size_t n, const uint64_t z[4], const uint64_t y[4], uint64_t* out_q_evals) {
    uint32_t lg = 0;
    if (!ctx || !evals || !z || !y || !out_q_evals || !ntt_log(n, &lg)) return KZG_ERR_INVALID_ARG;
    if (ctx->multi) return kzg_quotient_lagrange(multi_kid(ctx->multi, 0), evals, n, z, y, out_q_evals);  // needs no SRS
    std::unique_lock<std::mutex> lk(ctx->mu);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const int slot = reserve_slot(ctx, lk, true);
    if (slot < 0) return KZG_ERR_BUSY;
    SlotLease lease{ctx, slot};
    Slot& s = ctx->slots[slot];
    int rc = ensure_slot_basics(ctx, s);
    if (rc == KZG_OK) rc = lagrange_slot_ready(ctx, s, n, lg);
    if (rc == KZG_OK) rc = copy_unlocked(ctx, lk, s.stream, s.stage.dev(), evals, n * 32, hipMemcpyHostToDevice, "hipMemcpyAsync (evaluations)");
    if (rc == KZG_OK) rc = enqueue_lagrange_quotient(ctx, s, s.stage.dev(), lg, z, y);
    if (rc == KZG_OK) rc = sync_unlocked(ctx, lk, s.stream, "lagrange quotient");
    if (rc) return rc;
    const uint32_t* hs = s.small.host();
    if (!(hs[0] & 1u)) {  // every value equals f_0: a constant polynomial, whose quotient is zero when the claim holds
        if (std::memcmp(hs + 16, y, 32) != 0) return KZG_ERR_CONSTANT_POLY;
    } else if (std::memcmp(hs + 8, y, 32) != 0) {
        return KZG_ERR_REMAINDER;
    }
    rc = copy_unlocked(ctx, lk, s.stream, out_q_evals, s.q.dev(), n * 32, hipMemcpyDeviceToHost, "hipMemcpyAsync (quotient values)");
    if (rc == KZG_OK) rc = sync_unlocked(ctx, lk, s.stream, "lagrange quotient");
    return rc;
}

// ---- running products and running sums (grand_product_kernels.hip; lookup_kernels.hip, section 4.21) ----
//     products:  z_0 = 1,   z_(i+1) = z_i A_i / B_i              sums:  phi_0 = 0,   phi_(i+1) = phi_i + sum_j a_j[i] / b_j[i]
// One description for every form of either and one call frame per kind of entry point.  A call reserves gp_flags, gp_part, gp_in and
// gp_z on its slot, runs three kernels on the slot's stream (run_enqueue: the one step that differs between the forms) and reads
// the flag words: [0] the least index with a zero denominator (kGpNone = kLuNone: none), [8..15] the last value.
enum RunForm { kGpGeneral = 0, kGpPerm, kLuGeneral, kLuLookupForm, kLuInverse };
struct RunCall {  // the columns are host or device pointers as the caller's entry point says
    RunForm form;
    const void* a;         // products: the numerators, or the wires; sum: the numerators (may be null); lookup: the k lookup columns
    const void* b;         // products: the denominators, or the sigmas; sum: the denominators; inverse: the values
    const void *table, *mult;  // lookup form
    const uint64_t* beta;  // lookup and permutation forms
    size_t n, t, stride;   // t: columns of a and b (lookup form: k)
    const uint64_t *shifts, *gamma;  // permutation form
    uint32_t lg;                     // n = 2^lg: the permutation form and the commit calls
    bool product() const { return form <= kGpPerm; }
    const char* what() const { return product() ? "grand product" : "log-derivative sum"; }
    const char* out_what() const { return product() ? "hipMemcpyAsync (z)" : "hipMemcpyAsync (phi)"; }
};
static_assert(kGpNone == kLuNone, "one convention for the flag word of both kinds");
static bool run_shape_ok(size_t n, size_t t, size_t stride, size_t t_max) {
    return n >= 1 && n <= ((size_t)1 << kNttMaxLog) && t >= 1 && t <= t_max && stride >= n;
}
// the columns a host-pointer call packs into the slot (stride n)
static size_t run_packed_columns(const RunCall& c) {
    return c.form == kLuLookupForm ? c.t + 2 : (c.form == kLuInverse ? 1 : (c.a ? 2 : 1) * c.t);
}
// the slot's buffers (ctx->mu held, slot reserved); packed: a host-pointer call; own_out: the output goes to the slot's gp_z
static int run_slot_ready(kzg_ctx* ctx, Slot& s, const RunCall& c, bool packed, bool own_out) {
    const size_t part = c.product() ? (size_t)gp_tiles(c.n) * kGpPartialWords : (size_t)lu_tiles(c.n) * kLuPartialWords;
    int rc = ensure_slot_basics(ctx, s);
    if (rc == KZG_OK) rc = s.gp_flags.reserve(ctx, 64);
    if (rc == KZG_OK) rc = s.gp_part.reserve(ctx, part * 4, s.stream);
    if (rc == KZG_OK && packed) rc = s.gp_in.reserve(ctx, run_packed_columns(c) * c.n * 32, s.stream);
    if (rc == KZG_OK && own_out) rc = s.gp_z.reserve(ctx, c.n * 32, s.stream);
    return rc;
}
// t columns of n values each, column j at src + 4 j stride, packed to stride n at dst (the slot's stream, ctx->mu dropped meanwhile)
static int upload_columns(kzg_ctx* ctx, std::unique_lock<std::mutex>& lk, Slot& s, uint32_t* dst, const uint64_t* src, size_t n, size_t t,
                          size_t stride) {
    if (stride == n) return copy_unlocked(ctx, lk, s.stream, dst, src, t * n * 32, hipMemcpyHostToDevice, "hipMemcpyAsync (columns)");
    for (size_t j = 0; j < t; j++) {
        int rc = copy_unlocked(ctx, lk, s.stream, dst + 8 * j * n, src + 4 * j * stride, n * 32, hipMemcpyHostToDevice,
                               "hipMemcpyAsync (columns)");
        if (rc) return rc;
    }
    return KZG_OK;
}
// the three kernels of a call on device columns on the slot's stream: the output into d_out, the results into the slot's gp_flags
static int run_enqueue(kzg_ctx* ctx, Slot& s, const RunCall& c, uint32_t* d_out) {
    const size_t cols = c.form == kLuLookupForm ? c.t + 1 : (c.form == kLuInverse ? 1 : c.t);
    const Fr30 scale = fr30_arg_from_mont256(fr_pow2((uint32_t)(14 * cols)));  // 2^(270 + 14 cols): cols images -> one multiplier
    auto image = [](const uint64_t* v) {
        uint32_t l[8];
        std::memcpy(l, v, 32);
        return fr30_from_limbs(l);
    };
    const Fr30 one = image(hf::kFrOne.l);
    const uint32_t *a = (const uint32_t*)c.a, *b = (const uint32_t*)c.b, n = (uint32_t)c.n, t = (uint32_t)c.t;
    const GpOut gp_out{d_out, s.gp_part.dev(), s.gp_flags.dev()};
    const LuOut lu_out{d_out, s.gp_part.dev(), s.gp_flags.dev()};
    if (c.form == kGpGeneral) {
        launch_grand_product(s.stream, a, b, n, t, c.stride, scale, one, gp_out);
    } else if (c.form == kGpPerm) {
        hf::Fr beta, k;
        std::memcpy(beta.l, c.beta, 32);
        Fr30 bk[kGpMaxColumns];
        for (size_t j = 0; j < c.t; j++) {
            std::memcpy(k.l, c.shifts + 4 * j, 32);
            bk[j] = image(hf::fr_mul(beta, k).l);  // an image: its product with the twiddle (a multiplier) is added to f_j[i]
        }
        launch_permutation_product(s.stream, a, b, c.lg, t, c.stride, bk, fr30_arg_from_mont256(beta), image(c.gamma), ctx->ntt_tw.p, scale,
                                   one, gp_out);
    } else if (c.form == kLuGeneral) {
        launch_logderivative_sum(s.stream, a, b, n, t, c.stride, scale, one, lu_out);
    } else if (c.form == kLuLookupForm) {
        launch_lookup_sum(s.stream, a, n, t, c.stride, (const uint32_t*)c.table, (const uint32_t*)c.mult, image(c.beta), scale, one, lu_out);
    } else {
        launch_batch_inverse(s.stream, b, n, scale, one, lu_out);
    }
    HIP_TRY(ctx, hipGetLastError());
    return KZG_OK;
}
// a host-pointer call's columns packed into s.gp_in, then the kernels on those device columns
static int run_packed(kzg_ctx* ctx, std::unique_lock<std::mutex>& lk, Slot& s, const RunCall& c, uint32_t* d_out) {
    uint32_t* d = s.gp_in.dev();
    const size_t n = c.n, t = c.t;
    RunCall dev = c;
    dev.stride = n;
    int rc = KZG_OK;
    if (c.form == kLuLookupForm) {
        dev.a = d;
        dev.table = d + 8 * t * n;
        dev.mult = d + 8 * (t + 1) * n;
        rc = upload_columns(ctx, lk, s, d, (const uint64_t*)c.a, n, t, c.stride);
        if (rc == KZG_OK) rc = upload_columns(ctx, lk, s, d + 8 * t * n, (const uint64_t*)c.table, n, 1, n);
        if (rc == KZG_OK) rc = upload_columns(ctx, lk, s, d + 8 * (t + 1) * n, (const uint64_t*)c.mult, n, 1, n);
    } else if (c.form == kLuInverse) {
        dev.b = d;
        rc = upload_columns(ctx, lk, s, d, (const uint64_t*)c.b, n, 1, n);
    } else {  // two column sets, or the denominators alone
        dev.b = d;
        rc = upload_columns(ctx, lk, s, d, (const uint64_t*)c.b, n, t, c.stride);
        if (rc == KZG_OK && c.a) {
            dev.a = d + 8 * t * n;
            rc = upload_columns(ctx, lk, s, d + 8 * t * n, (const uint64_t*)c.a, n, t, c.stride);
        }
    }
    return rc ? rc : run_enqueue(ctx, s, dev, d_out);
}
// after the stream was waited for: the status of the call, the last value (out_last null: the inverse form, which has none), the
// index of a zero denominator
static int run_result(kzg_ctx* ctx, const Slot& s, const RunCall& c, uint64_t out_last[4], size_t* bad_index) {
    const uint32_t* h = s.gp_flags.host();
    if (bad_index) *bad_index = h[0] == kGpNone ? (size_t)-1 : (size_t)h[0];
    if (h[0] != kGpNone) {
        const char* sum = c.form == kLuInverse ? "batch inverse: the value at row " : "log-derivative sum: a denominator at row ";
        ctx->last_error = (c.product() ? "grand product: the denominator at index " : sum) + std::to_string(h[0]) + " is zero";
        return KZG_ERR_INVALID_ARG;
    }
    if (out_last) std::memcpy(out_last, h + 8, 32);
    return KZG_OK;
}
// a host-pointer call: the columns packed into the slot, the output back through the slot's gp_z
static int run_host(kzg_ctx* ctx, const RunCall& c, uint64_t* out, uint64_t out_last[4], size_t* bad_index) {
    std::unique_lock<std::mutex> lk(ctx->mu);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    int rc = c.form == kGpPerm ? ensure_ntt(ctx) : KZG_OK;
    if (rc) return rc;
    const int slot = reserve_slot(ctx, lk, true);
    if (slot < 0) return KZG_ERR_BUSY;
    SlotLease lease{ctx, slot};
    Slot& s = ctx->slots[slot];
    rc = run_slot_ready(ctx, s, c, true, true);
    if (rc == KZG_OK) rc = run_packed(ctx, lk, s, c, s.gp_z.dev());
    if (rc == KZG_OK) rc = copy_unlocked(ctx, lk, s.stream, out, s.gp_z.dev(), c.n * 32, hipMemcpyDeviceToHost, c.out_what());
    if (rc == KZG_OK) rc = sync_unlocked(ctx, lk, s.stream, c.what());
    return rc ? rc : run_result(ctx, s, c, out_last, bad_index);
}
static bool ranges_overlap(const void* out, size_t out_bytes, const void* in, size_t in_bytes) {  // (a null input overlaps nothing)
    return in && (const char*)out < (const char*)in + in_bytes && (const char*)in < (const char*)out + out_bytes;
}
// a call on device columns on a slot the caller holds, with the context's mutex (*lk), the device current and the twiddles built
// where the form reads them: the body of run_device, and a step of the circuit calls (sections 4.24, 4.26)
static int run_on_slot(kzg_ctx* ctx, std::unique_lock<std::mutex>& lk, Slot& s, const RunCall& c, void* d_out, uint64_t out_last[4],
                       size_t* bad_index) {
    int rc = run_slot_ready(ctx, s, c, false, false);
    if (rc == KZG_OK) rc = run_enqueue(ctx, s, c, (uint32_t*)d_out);
    if (rc == KZG_OK) rc = sync_unlocked(ctx, lk, s.stream, c.what());
    return rc ? rc : run_result(ctx, s, c, out_last, bad_index);
}
static int run_device(kzg_ctx* ctx, const RunCall& c, void* d_out, uint64_t out_last[4], size_t* bad_index) {
    const size_t span = ((c.t - 1) * c.stride + c.n) * 32, one = c.n * 32;  // bytes a column set covers, bytes of one column
    const bool columns = c.form != kLuInverse;
    if ((columns && ranges_overlap(d_out, one, c.a, span)) || ranges_overlap(d_out, one, c.b, columns ? span : one) ||
        ranges_overlap(d_out, one, c.table, one) || ranges_overlap(d_out, one, c.mult, one)) {
        ctx->last_error = std::string(c.what()) + ": the output overlaps an input";
        return KZG_ERR_INVALID_ARG;
    }
    std::unique_lock<std::mutex> lk(ctx->mu);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    int rc = c.form == kGpPerm ? ensure_ntt(ctx) : KZG_OK;
    if (rc) return rc;
    const int slot = reserve_slot(ctx, lk, true);
    if (slot < 0) return KZG_ERR_BUSY;
    SlotLease lease{ctx, slot};
    return run_on_slot(ctx, lk, ctx->slots[slot], c, d_out, out_last, bad_index);
}
// a host-pointer call whose output is also committed over the Lagrange basis of n = 2^lg points: it goes to the slot's staging
// buffer, where the MSM reads it, and comes back to the host only where `out` is given
static int run_commit(kzg_ctx* ctx, const RunCall& c, uint64_t* out, uint64_t out_last[4], uint64_t out_p1[18], size_t* bad_index) {
    std::unique_lock<std::mutex> lk(ctx->mu);
    int rc = lagrange_ensure(ctx, lk, c.n, c.lg);
    if (rc) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    rc = c.form == kGpPerm ? ensure_ntt(ctx) : KZG_OK;
    if (rc) return rc;
    const int slot = reserve_slot(ctx, lk, true);
    if (slot < 0) return KZG_ERR_BUSY;
    SlotLease lease{ctx, slot};  // (the basis stays until the submit, as for kzg_commit_lagrange)
    Slot& s = ctx->slots[slot];
    rc = run_slot_ready(ctx, s, c, true, false);
    if (rc == KZG_OK) rc = ensure_poly(ctx, s, c.n);
    if (rc) return rc;
    rc = run_packed(ctx, lk, s, c, s.stage.dev());
    if (rc == KZG_OK && out) rc = copy_unlocked(ctx, lk, s.stream, out, s.stage.dev(), c.n * 32, hipMemcpyDeviceToHost, c.out_what());
    MsmBasis basis{};
    if (rc == KZG_OK && !lagrange_basis(ctx, c.n, &basis)) rc = KZG_ERR_NO_SRS;
    if (rc == KZG_OK) rc = submit_commit_locked(ctx, slot, s.stage.dev(), 1, c.n, true, true, &basis);
    if (rc) return rc;
    await_unlocked(lk, s);
    rc = wait_locked(ctx, slot, out_p1);
    return rc ? rc : run_result(ctx, s, c, out_last, bad_index);
}

int kzg_grand_product(kzg_ctx* ctx, const uint64_t* nums, const uint64_t* dens, size_t n, size_t t, size_t stride, uint64_t* out_z,
                      uint64_t out_last[4], size_t* bad_index) {
    if (!ctx || !nums || !dens || !out_z || !out_last || !run_shape_ok(n, t, stride, kGpMaxColumns)) return KZG_ERR_INVALID_ARG;
    if (ctx->multi) {  // needs no SRS
        kzg_ctx* kid = multi_kid(ctx->multi, 0);
        return forwarded(ctx, kid, kzg_grand_product(kid, nums, dens, n, t, stride, out_z, out_last, bad_index));
    }
    return run_host(ctx, RunCall{kGpGeneral, nums, dens, nullptr, nullptr, nullptr, n, t, stride}, out_z, out_last, bad_index);
}

int kzg_grand_product_device(kzg_ctx* ctx, const void* d_nums, const void* d_dens, size_t n, size_t t, size_t stride, void* d_out_z,
                             uint64_t out_last[4], size_t* bad_index) {
    KZG_SINGLE_DEVICE_ONLY(ctx);
    if (!ctx || !d_nums || !d_dens || !d_out_z || !out_last || !run_shape_ok(n, t, stride, kGpMaxColumns)) return KZG_ERR_INVALID_ARG;
    return run_device(ctx, RunCall{kGpGeneral, d_nums, d_dens, nullptr, nullptr, nullptr, n, t, stride}, d_out_z, out_last, bad_index);
}

int kzg_permutation_product(kzg_ctx* ctx, const uint64_t* wires, const uint64_t* sigmas, size_t n, size_t t, size_t stride,
                            const uint64_t* shifts, const uint64_t beta[4], const uint64_t gamma[4], uint64_t* out_z,
                            uint64_t out_last[4], size_t* bad_index) {
    uint32_t lg = 0;
    if (!ctx || !wires || !sigmas || !shifts || !beta || !gamma || !out_z || !out_last || !run_shape_ok(n, t, stride, kGpMaxColumns) ||
        !ntt_log(n, &lg))
        return KZG_ERR_INVALID_ARG;
    if (ctx->multi) {  // needs no SRS
        kzg_ctx* kid = multi_kid(ctx->multi, 0);
        return forwarded(ctx, kid, kzg_permutation_product(kid, wires, sigmas, n, t, stride, shifts, beta, gamma, out_z, out_last, bad_index));
    }
    return run_host(ctx, RunCall{kGpPerm, wires, sigmas, nullptr, nullptr, beta, n, t, stride, shifts, gamma, lg}, out_z, out_last, bad_index);
}

int kzg_permutation_product_device(kzg_ctx* ctx, const void* d_wires, const void* d_sigmas, size_t n, size_t t, size_t stride,
                                   const uint64_t* shifts, const uint64_t beta[4], const uint64_t gamma[4], void* d_out_z,
                                   uint64_t out_last[4], size_t* bad_index) {
    KZG_SINGLE_DEVICE_ONLY(ctx);
    uint32_t lg = 0;
    if (!ctx || !d_wires || !d_sigmas || !shifts || !beta || !gamma || !d_out_z || !out_last ||
        !run_shape_ok(n, t, stride, kGpMaxColumns) || !ntt_log(n, &lg))
        return KZG_ERR_INVALID_ARG;
    return run_device(ctx, RunCall{kGpPerm, d_wires, d_sigmas, nullptr, nullptr, beta, n, t, stride, shifts, gamma, lg}, d_out_z, out_last,
                      bad_index);
}

int kzg_permutation_commit(kzg_ctx* ctx, const uint64_t* wires, const uint64_t* sigmas, size_t n, size_t t, size_t stride,
                           const uint64_t* shifts, const uint64_t beta[4], const uint64_t gamma[4], uint64_t* out_z,
                           uint64_t out_last[4], uint64_t out_p1[18], size_t* bad_index) {
    uint32_t lg = 0;
    if (!ctx || !wires || !sigmas || !shifts || !beta || !gamma || !out_last || !out_p1 || !run_shape_ok(n, t, stride, kGpMaxColumns) ||
        !ntt_log(n, &lg))
        return KZG_ERR_INVALID_ARG;
    if (ctx->multi) {
        int rc = KZG_OK;
        kzg_ctx* kid = lagrange_kid(ctx, &rc);
        return kid ? forwarded(ctx, kid, kzg_permutation_commit(kid, wires, sigmas, n, t, stride, shifts, beta, gamma, out_z, out_last,
                                                                 out_p1, bad_index))
                   : rc;
    }
    return run_commit(ctx, RunCall{kGpPerm, wires, sigmas, nullptr, nullptr, beta, n, t, stride, shifts, gamma, lg}, out_z, out_last, out_p1,
                      bad_index);
}

int kzg_logderivative_sum(kzg_ctx* ctx, const uint64_t* nums, const uint64_t* dens, size_t n, size_t t, size_t stride, uint64_t* out_phi,
                          uint64_t out_last[4], size_t* bad_index) {
    if (!ctx || !dens || !out_phi || !out_last || !run_shape_ok(n, t, stride, kLuMaxColumns)) return KZG_ERR_INVALID_ARG;
    if (ctx->multi) {  // needs no SRS
        kzg_ctx* kid = multi_kid(ctx->multi, 0);
        return forwarded(ctx, kid, kzg_logderivative_sum(kid, nums, dens, n, t, stride, out_phi, out_last, bad_index));
    }
    return run_host(ctx, RunCall{kLuGeneral, nums, dens, nullptr, nullptr, nullptr, n, t, stride}, out_phi, out_last, bad_index);
}

int kzg_logderivative_sum_device(kzg_ctx* ctx, const void* d_nums, const void* d_dens, size_t n, size_t t, size_t stride, void* d_out_phi,
                                 uint64_t out_last[4], size_t* bad_index) {
    if (!ctx || !d_dens || !d_out_phi || !out_last || !run_shape_ok(n, t, stride, kLuMaxColumns)) return KZG_ERR_INVALID_ARG;
    KZG_SINGLE_DEVICE_ONLY(ctx);
    return run_device(ctx, RunCall{kLuGeneral, d_nums, d_dens, nullptr, nullptr, nullptr, n, t, stride}, d_out_phi, out_last, bad_index);
}

int kzg_lookup_sum(kzg_ctx* ctx, const uint64_t* lookups, size_t n, size_t k, size_t stride, const uint64_t* table, const uint64_t* mult,
                   const uint64_t beta[4], uint64_t* out_phi, uint64_t out_last[4], size_t* bad_index) {
    if (!ctx || !lookups || !table || !mult || !beta || !out_phi || !out_last || !run_shape_ok(n, k, stride, kLuMaxColumns - 1))
        return KZG_ERR_INVALID_ARG;
    if (ctx->multi) {  // needs no SRS
        kzg_ctx* kid = multi_kid(ctx->multi, 0);
        return forwarded(ctx, kid, kzg_lookup_sum(kid, lookups, n, k, stride, table, mult, beta, out_phi, out_last, bad_index));
    }
    return run_host(ctx, RunCall{kLuLookupForm, lookups, nullptr, table, mult, beta, n, k, stride}, out_phi, out_last, bad_index);
}

int kzg_lookup_sum_device(kzg_ctx* ctx, const void* d_lookups, size_t n, size_t k, size_t stride, const void* d_table, const void* d_mult,
                          const uint64_t beta[4], void* d_out_phi, uint64_t out_last[4], size_t* bad_index) {
    if (!ctx || !d_lookups || !d_table || !d_mult || !beta || !d_out_phi || !out_last || !run_shape_ok(n, k, stride, kLuMaxColumns - 1))
        return KZG_ERR_INVALID_ARG;
    KZG_SINGLE_DEVICE_ONLY(ctx);
    return run_device(ctx, RunCall{kLuLookupForm, d_lookups, nullptr, d_table, d_mult, beta, n, k, stride}, d_out_phi, out_last, bad_index);
}

int kzg_batch_inverse(kzg_ctx* ctx, const uint64_t* vals, size_t n, uint64_t* out, size_t* bad_index) {
    if (!ctx || !vals || !out || !run_shape_ok(n, 1, n, 1)) return KZG_ERR_INVALID_ARG;
    if (ctx->multi) {  // needs no SRS
        kzg_ctx* kid = multi_kid(ctx->multi, 0);
        return forwarded(ctx, kid, kzg_batch_inverse(kid, vals, n, out, bad_index));
    }
    return run_host(ctx, RunCall{kLuInverse, nullptr, vals, nullptr, nullptr, nullptr, n, 1, n}, out, nullptr, bad_index);
}

int kzg_batch_inverse_device(kzg_ctx* ctx, const void* d_vals, size_t n, void* d_out, size_t* bad_index) {
    if (!ctx || !d_vals || !d_out || !run_shape_ok(n, 1, n, 1)) return KZG_ERR_INVALID_ARG;
    KZG_SINGLE_DEVICE_ONLY(ctx);
    return run_device(ctx, RunCall{kLuInverse, nullptr, d_vals, nullptr, nullptr, nullptr, n, 1, n}, d_out, nullptr, bad_index);
}

int kzg_lookup_commit(kzg_ctx* ctx, const uint64_t* lookups, size_t n, size_t k, size_t stride, const uint64_t* table, const uint64_t* mult,
                      const uint64_t beta[4], uint64_t* out_phi, uint64_t out_last[4], uint64_t out_p1[18], size_t* bad_index) {
    uint32_t lg = 0;
    if (!ctx || !lookups || !table || !mult || !beta || !out_last || !out_p1 || !run_shape_ok(n, k, stride, kLuMaxColumns - 1) ||
        !ntt_log(n, &lg))
        return KZG_ERR_INVALID_ARG;
    if (ctx->multi) {
        int rc = KZG_OK;
        kzg_ctx* kid = lagrange_kid(ctx, &rc);
        return kid ? forwarded(ctx, kid, kzg_lookup_commit(kid, lookups, n, k, stride, table, mult, beta, out_phi, out_last, out_p1, bad_index))
                   : rc;
    }
    return run_commit(ctx, RunCall{kLuLookupForm, lookups, nullptr, table, mult, beta, n, k, stride, nullptr, nullptr, lg}, out_phi, out_last,
                      out_p1, bad_index);
}

// ---- multiplicities of a lookup through a hash table on the device (lookup_kernels.hip) -------------------
// A call holds lookup_mu, then the context's mutex and one slot for its stream, dropping the mutex while it copies or waits.
namespace {
enum : int { kLuWsTable = 0, kLuWsLookups, kLuWsSlots, kLuWsCounts, kLuWsMult, kLuWsRows, kLuWsCount };
static_assert(kLuWsCount <= 6, "lu_ws");
// Declared after the slot's lease, so that it runs first: nothing the call enqueued still uses lu_ws when lookup_mu is given up.
struct LuDrain {
    const Slot& s;
    ~LuDrain() {
        if (s.stream) (void)hipStreamSynchronize(s.stream);
    }
};
bool lu_mult_shape(size_t n_table, size_t n, size_t k, size_t stride) {
    const size_t top = (size_t)1 << kNttMaxLog;
    return n_table >= 1 && n_table <= top && n >= 1 && n <= top && k >= 1 && k <= kLuMaxColumns - 1 && stride >= n;
}
// the least power of two >= 2 n_table
unsigned lu_default_log_capacity(size_t n_table) {
    unsigned lg = 1;
    while (((size_t)1 << lg) < 2 * n_table) lg++;
    return lg;
}
// The hash table and the kernels of one call on device columns, on the stream of a slot the caller holds with lookup_mu and the
// context's mutex; the verdict is in the slot's gp_flags once the stream was waited for (lu_mult_verdict)
int lu_mult_enqueue(kzg_ctx* ctx, Slot& s, const void* d_table, size_t n_table, const void* d_look, size_t n, size_t k, size_t stride,
                    unsigned log_cap, void* d_mult, void* d_rows) {
    const size_t cap = (size_t)1 << log_cap;
    void *d_slots = nullptr, *d_counts = nullptr;
    int rc = ctx->lu_ws.get(ctx, kLuWsSlots, (cap + 4) * 4, &d_slots);  // the slots, then the two flag words
    if (rc == KZG_OK) rc = ctx->lu_ws.get(ctx, kLuWsCounts, n_table * 4, &d_counts);
    if (rc) return rc;
    HIP_TRY(ctx, hipMemsetAsync(d_slots, 0xff, (cap + 4) * 4, s.stream));
    HIP_TRY(ctx, hipMemsetAsync(d_counts, 0, n_table * 4, s.stream));
    const LuHash h{(uint32_t*)d_slots, log_cap, (uint32_t*)d_counts, (uint32_t*)d_slots + cap};
    launch_lookup_multiplicities(s.stream, (const uint32_t*)d_table, (uint32_t)n_table, (const uint32_t*)d_look, (uint32_t)n, (uint32_t)k,
                                 stride, h, fr30_arg_from_mont256(fr_pow2(256)), (uint32_t*)d_mult, (uint32_t*)d_rows, s.gp_flags.dev());
    HIP_TRY(ctx, hipGetLastError());
    return KZG_OK;
}
int lu_mult_verdict(kzg_ctx* ctx, const Slot& s, size_t* bad_index) {
    const uint32_t* f = s.gp_flags.host();
    if (bad_index) *bad_index = f[0] == kLuNone ? (size_t)-1 : (size_t)f[0];
    if (f[1] != kLuNone) {  // not reached with a capacity >= n_table
        ctx->last_error = "lookup multiplicities: the hash table is full at table row " + std::to_string(f[1]);
        return KZG_ERR_INVALID_ARG;
    }
    if (f[0] != kLuNone) {
        ctx->last_error = "lookup multiplicities: a value at row " + std::to_string(f[0]) + " of the lookup columns is in no table row";
        return KZG_ERR_INVALID_ARG;
    }
    return KZG_OK;
}
int lu_multiplicities(kzg_ctx* ctx, const void* table, size_t n_table, const void* lookups, size_t n, size_t k, size_t stride, void* out_mult,
                      void* out_rows, size_t* bad_index, unsigned log_cap, bool device) {
    std::lock_guard<std::mutex> lkl(ctx->lookup_mu);
    std::unique_lock<std::mutex> lk(ctx->mu);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const int slot = reserve_slot(ctx, lk, true);
    if (slot < 0) return KZG_ERR_BUSY;
    SlotLease lease{ctx, slot};
    Slot& s = ctx->slots[slot];
    LuDrain drain{s};
    int rc = ensure_slot_basics(ctx, s);
    if (rc == KZG_OK) rc = s.gp_flags.reserve(ctx, 64);
    void *d_table = (void*)table, *d_look = (void*)lookups, *d_mult = out_mult, *d_rows = out_rows;
    if (!device) {
        if (rc == KZG_OK) rc = ctx->lu_ws.get(ctx, kLuWsTable, n_table * 32, &d_table);
        if (rc == KZG_OK) rc = ctx->lu_ws.get(ctx, kLuWsLookups, k * n * 32, &d_look);
        if (rc == KZG_OK) rc = ctx->lu_ws.get(ctx, kLuWsMult, n_table * 32, &d_mult);
        if (rc == KZG_OK && out_rows) rc = ctx->lu_ws.get(ctx, kLuWsRows, k * n * 4, &d_rows);
        if (rc == KZG_OK) rc = copy_unlocked(ctx, lk, s.stream, d_table, table, n_table * 32, hipMemcpyHostToDevice, "hipMemcpyAsync (table)");
        if (rc == KZG_OK) rc = upload_columns(ctx, lk, s, (uint32_t*)d_look, (const uint64_t*)lookups, n, k, stride);
    }
    if (rc == KZG_OK) rc = lu_mult_enqueue(ctx, s, d_table, n_table, d_look, n, k, device ? stride : n, log_cap, d_mult, d_rows);
    if (rc) return rc;
    if (!device) {
        rc = copy_unlocked(ctx, lk, s.stream, out_mult, d_mult, n_table * 32, hipMemcpyDeviceToHost, "hipMemcpyAsync (multiplicities)");
        if (rc == KZG_OK && out_rows)
            rc = copy_unlocked(ctx, lk, s.stream, out_rows, d_rows, k * n * 4, hipMemcpyDeviceToHost, "hipMemcpyAsync (rows)");
    }
    if (rc == KZG_OK) rc = sync_unlocked(ctx, lk, s.stream, "lookup multiplicities");
    return rc ? rc : lu_mult_verdict(ctx, s, bad_index);
}
}  // namespace

int kzg_lookup_multiplicities_cap(kzg_ctx* ctx, const uint64_t* table, size_t n_table, const uint64_t* lookups, size_t n, size_t k,
                                  size_t stride, uint64_t* out_mult, uint32_t* out_rows, size_t* bad_index, unsigned log_capacity) {
    if (!ctx || !table || !lookups || !out_mult || !lu_mult_shape(n_table, n, k, stride) || log_capacity > kNttMaxLog + 1 ||
        ((size_t)1 << log_capacity) < n_table)
        return KZG_ERR_INVALID_ARG;
    if (ctx->multi) {  // needs no SRS
        kzg_ctx* kid = multi_kid(ctx->multi, 0);
        return forwarded(ctx, kid, kzg_lookup_multiplicities_cap(kid, table, n_table, lookups, n, k, stride, out_mult, out_rows, bad_index,
                                                                 log_capacity));
    }
    return lu_multiplicities(ctx, table, n_table, lookups, n, k, stride, out_mult, out_rows, bad_index, log_capacity, false);
}

int kzg_lookup_multiplicities(kzg_ctx* ctx, const uint64_t* table, size_t n_table, const uint64_t* lookups, size_t n, size_t k, size_t stride,
                              uint64_t* out_mult, uint32_t* out_rows, size_t* bad_index) {
    if (!ctx || !lu_mult_shape(n_table, n, k, stride)) return KZG_ERR_INVALID_ARG;
    return kzg_lookup_multiplicities_cap(ctx, table, n_table, lookups, n, k, stride, out_mult, out_rows, bad_index,
                                         lu_default_log_capacity(n_table));
}

int kzg_lookup_multiplicities_device(kzg_ctx* ctx, const void* d_table, size_t n_table, const void* d_lookups, size_t n, size_t k,
                                     size_t stride, void* d_out_mult, void* d_out_rows, size_t* bad_index) {
    if (!ctx || !d_table || !d_lookups || !d_out_mult || !lu_mult_shape(n_table, n, k, stride)) return KZG_ERR_INVALID_ARG;
    KZG_SINGLE_DEVICE_ONLY(ctx);
    const size_t span = ((k - 1) * stride + n) * 32;
    for (const void* out : {(const void*)d_out_mult, (const void*)d_out_rows}) {
        const size_t bytes = out == d_out_mult ? n_table * 32 : k * n * 4;
        if (out && (ranges_overlap(out, bytes, d_table, n_table * 32) || ranges_overlap(out, bytes, d_lookups, span) ||
                    (out == d_out_rows && ranges_overlap(out, bytes, d_out_mult, n_table * 32)))) {
            ctx->last_error = "lookup multiplicities: an output overlaps an input or the other output";
            return KZG_ERR_INVALID_ARG;
        }
    }
    return lu_multiplicities(ctx, d_table, n_table, d_lookups, n, k, stride, d_out_mult, d_out_rows, bad_index,
                             lu_default_log_capacity(n_table), true);
}

// ---- recovery of every cell and proof from part of the cells (recover_kernels.hip) -----------------
// The decode holds recover_mu, then the context's mutex and one slot for its stream, dropping the mutex while it waits for the
// device; the cells come from the same pass.  Proofs go through fk20_host afterwards with the recovered coefficients (one more
// upload of them).
namespace {
enum : int { kRecIn = 0, kRecA, kRecB, kRecCoef, kRecFlags, kRecPos, kRecMissing, kRecPart, kRecZ, kRecWire, kRecErr, kRecCount };
// the byte-string form of a recovery (section 4.13): the received cells as they travel, decoded on the device; the cells leave
// encoded; the coefficients of the whole batch stay in device memory (d_coeffs: batch x n x 32 bytes) for FK20
struct RecWire {
    const uint8_t* cells_be = nullptr;
    bool bit_reversed = false;
    const uint32_t* ids_sent = nullptr;  // the caller's cell ids, for the message that names a value
    uint8_t* out_cells_be = nullptr;
    void* d_coeffs = nullptr;
};
constexpr size_t kRecMaxBatch = 64;               // polynomials per pass through the workspaces, at most
constexpr size_t kRecWsBudget = (size_t)2 << 30;  // ... and fewer when their workspaces would pass this
hf::Fr fr_seven() {
    hf::Fr g = hf::kFrOne;
    for (int i = 0; i < 6; i++) g = hf::fr_add(g, hf::kFrOne);
    return g;
}
}  // namespace

// g^i and g^-i tables (ctx->mu held, device current): forward lo, forward hi, inverse lo, inverse hi, as ensure_ntt's
static int ensure_recover_g(kzg_ctx* ctx) {
    if (ctx->rec_g.p) return KZG_OK;
    std::vector<Fr30> h(4 * kNttTableLen);
    const hf::Fr g = fr_seven();
    for (int dir = 0; dir < 2; dir++) {
        const hf::Fr base = dir ? hf::fr_inv(g) : g;
        const hf::Fr step_hi = hf::fr_pow(base, kNttTableLen);
        hf::Fr lo = hf::kFrOne, hi = hf::kFrOne;
        for (uint32_t i = 0; i < kNttTableLen; i++) {
            h[2 * dir * kNttTableLen + i] = fr30_arg_from_mont256(lo);
            h[(2 * dir + 1) * kNttTableLen + i] = fr30_arg_from_mont256(hi);
            lo = hf::fr_mul(lo, base);
            hi = hf::fr_mul(hi, step_hi);
        }
    }
    DevBuf d;
    HIP_TRY(ctx, hipMalloc(&d.p, h.size() * sizeof(Fr30)));
    if (hipError_t e = hipMemcpy(d.p, h.data(), h.size() * sizeof(Fr30), hipMemcpyHostToDevice))
        return hip_fail(ctx, "hipMemcpy (recovery tables)", e);
    std::swap(ctx->rec_g.p, d.p);
    return KZG_OK;
}

// the decode of `batch` validated polynomials: coefficients to out_coeffs, cells to out_cells (either may be null);
// KZG_ERR_REMAINDER names the first polynomial whose coefficients at [n, N) are not all zero
static int recover_host(kzg_ctx* ctx, const CellsShape& sh, size_t n, const int32_t* pos, const std::vector<uint32_t>& missing,
                        size_t k, const uint64_t* cells, size_t batch, uint64_t* out_coeffs, uint64_t* out_cells,
                        const RecWire* wire = nullptr) {
    std::lock_guard<std::mutex> lkr(ctx->recover_mu);
    std::unique_lock<std::mutex> lk(ctx->mu);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    int rc = ensure_ntt(ctx);
    if (rc == KZG_OK) rc = ensure_recover_g(ctx);
    if (rc) return rc;
    const int slot = reserve_slot(ctx, lk, true);
    if (slot < 0) return KZG_ERR_BUSY;
    SlotLease lease{ctx, slot};
    Slot& s = ctx->slots[slot];
    rc = ensure_slot_basics(ctx, s);  // needs no SRS
    if (rc) return rc;
    const size_t N = sh.N, M = sh.cells, l = sh.l;
    const size_t per_poly = 2 * N * 32 + n * 32;
    size_t chunk = kRecWsBudget / per_poly;
    chunk = chunk < 1 ? 1 : (chunk > kRecMaxBatch ? kRecMaxBatch : chunk);
    if (chunk > batch) chunk = batch;
    const uint32_t parts = recover_vanish_parts((uint32_t)missing.size());
    void *in, *a, *b, *coef, *flags, *dpos, *dmiss, *part, *z;
    rc = ctx->rec_ws.get(ctx, kRecIn, batch * k * l * 32, &in);
    if (rc == KZG_OK) rc = ctx->rec_ws.get(ctx, kRecA, chunk * N * 32, &a);
    if (rc == KZG_OK) rc = ctx->rec_ws.get(ctx, kRecB, chunk * N * 32, &b);
    if (rc == KZG_OK) rc = ctx->rec_ws.get(ctx, kRecCoef, chunk * n * 32, &coef);
    if (rc == KZG_OK) rc = ctx->rec_ws.get(ctx, kRecFlags, chunk * 4, &flags);
    if (rc == KZG_OK) rc = ctx->rec_ws.get(ctx, kRecPos, M * 4, &dpos);
    if (rc == KZG_OK) rc = ctx->rec_ws.get(ctx, kRecMissing, missing.size() * 4, &dmiss);
    if (rc == KZG_OK) rc = ctx->rec_ws.get(ctx, kRecPart, (size_t)parts * 2 * M * 32, &part);
    if (rc == KZG_OK) rc = ctx->rec_ws.get(ctx, kRecZ, 2 * M * 32, &z);
    if (rc) return rc;
    uint32_t* derr = nullptr;
    const bool want_cells = wire ? wire->out_cells_be != nullptr : out_cells != nullptr;
    if (wire) {  // the bytes as received -> blst_fr images in `in`, the values of every cell put into this API's order
        void *dwire, *e;
        rc = ctx->rec_ws.get(ctx, kRecWire, batch * k * l * 32, &dwire);
        if (rc == KZG_OK) rc = ctx->rec_ws.get(ctx, kRecErr, 8, &e);
        if (rc) return rc;
        derr = (uint32_t*)e;
        HIP_TRY(ctx, hipMemsetAsync(derr, 0xff, 8, s.stream));
        rc = copy_unlocked(ctx, lk, s.stream, dwire, wire->cells_be, batch * k * l * 32, hipMemcpyHostToDevice, "hipMemcpyAsync (cells)");
        if (rc) return rc;
        launch_wire_fr(s.stream, dwire, (uint32_t)(batch * k * l), sh.log_l, wire->bit_reversed, in, derr);
    } else {
        rc = copy_unlocked(ctx, lk, s.stream, in, cells, batch * k * l * 32, hipMemcpyHostToDevice, "hipMemcpyAsync (cells)");
    }
    if (rc == KZG_OK) rc = copy_unlocked(ctx, lk, s.stream, dpos, pos, M * 4, hipMemcpyHostToDevice, "hipMemcpyAsync (cells)");
    if (rc == KZG_OK) rc = copy_unlocked(ctx, lk, s.stream, dmiss, missing.data(), missing.size() * 4, hipMemcpyHostToDevice, "hipMemcpyAsync (cells)");
    if (rc) return rc;
    const Fr30 gl = fr30_arg_from_mont256(hf::fr_pow(fr_seven(), l));
    const Fr30 inv_n = fr30_arg_from_mont256(hf::fr_inv(fr_pow2(sh.log_n)));
    const Fr30* tw = (const Fr30*)ctx->ntt_tw.p;
    const Fr30* gt = (const Fr30*)ctx->rec_g.p;
    launch_recover_vanishing(s.stream, (const uint32_t*)dmiss, (uint32_t)missing.size(), tw, sh.log_n, sh.log_l, gl,
                             (uint32_t*)part, (uint32_t*)z);
    std::vector<uint32_t> hflags(chunk);
    uint32_t *A = (uint32_t*)a, *B = (uint32_t*)b;
    for (size_t b0 = 0; b0 < batch; b0 += chunk) {
        const size_t bc = batch - b0 < chunk ? batch - b0 : chunk;
        HIP_TRY(ctx, hipMemsetAsync(flags, 0, bc * 4, s.stream));
        launch_recover_scatter(s.stream, (const uint32_t*)in + 8 * b0 * k * l, (const int32_t*)dpos, (const uint32_t*)z, (uint32_t)k,
                               sh.log_n, sh.log_l, bc, A);
        uint32_t* cur = const_cast<uint32_t*>(launch_fr_dft(s.stream, A, A, B, sh.log_n, bc, tw + 2 * kNttTableLen));
        launch_recover_twist(s.stream, cur, sh.log_n, bc, gt, inv_n);
        cur = const_cast<uint32_t*>(launch_fr_dft(s.stream, cur, A, B, sh.log_n, bc, tw));
        launch_recover_divide(s.stream, cur, sh.log_n, sh.log_l, bc, (const uint32_t*)z + 8 * M);
        cur = const_cast<uint32_t*>(launch_fr_dft(s.stream, cur, A, B, sh.log_n, bc, tw + 2 * kNttTableLen));
        launch_recover_untwist(s.stream, cur, sh.log_n, (uint32_t)n, bc, gt + 2 * kNttTableLen, inv_n,
                               wire ? (uint32_t*)wire->d_coeffs + 8 * n * b0 : (uint32_t*)coef, want_cells, (uint32_t*)flags);
        const uint32_t* cells_dev = nullptr;
        if (want_cells) {
            const uint32_t* ev = launch_fr_dft(s.stream, cur, A, B, sh.log_n, bc, tw);
            uint32_t* dst = ev == A ? B : A;
            launch_recover_gather(s.stream, ev, dst, sh.log_n, sh.log_l, bc);
            cells_dev = dst;
            if (wire) {  // the transform's buffer is free: the cells' bytes go there (canonical values: the second word stays unset)
                uint32_t* enc = ev == A ? A : B;
                launch_enc_fr(s.stream, dst, (uint32_t)(bc * N), sh.log_l, sh.log_n - sh.log_l, wire->bit_reversed, enc, derr + 1);
                cells_dev = enc;
            }
        }
        HIP_TRY(ctx, hipGetLastError());
        rc = sync_unlocked(ctx, lk, s.stream, "recover");
        if (rc) return rc;
        uint32_t herr = 0xffffffffu;
        HIP_TRY(ctx, hipMemcpyAsync(hflags.data(), flags, bc * 4, hipMemcpyDeviceToHost, s.stream));
        if (wire) {
            HIP_TRY(ctx, hipMemcpyAsync(&herr, derr, 4, hipMemcpyDeviceToHost, s.stream));
            if (cells_dev) HIP_TRY(ctx, hipMemcpyAsync(wire->out_cells_be + 32 * N * b0, cells_dev, bc * N * 32, hipMemcpyDeviceToHost, s.stream));
        } else {
            if (out_coeffs) HIP_TRY(ctx, hipMemcpyAsync(out_coeffs + 4 * n * b0, coef, bc * n * 32, hipMemcpyDeviceToHost, s.stream));
            if (cells_dev) HIP_TRY(ctx, hipMemcpyAsync(out_cells + 4 * N * b0, cells_dev, bc * N * 32, hipMemcpyDeviceToHost, s.stream));
        }
        rc = sync_unlocked(ctx, lk, s.stream, "recover");
        if (rc) return rc;
        if (herr != 0xffffffffu) {  // (the whole batch was decoded in front of the first chunk)
            const size_t b = herr / (k * l), t = herr / l % k;
            ctx->last_error = "recover: polynomial " + std::to_string(b) + ", cell " + std::to_string(wire->ids_sent[t]) + ": value " +
                              std::to_string(herr % l) + " is not below r";
            return KZG_ERR_INVALID_ARG;
        }
        for (size_t i = 0; i < bc; i++)
            if (hflags[i]) {
                ctx->last_error = "recover: polynomial " + std::to_string(b0 + i) + ": the received values are not those of a "
                                  "polynomial of fewer than " + std::to_string(n) + " coefficients";
                return KZG_ERR_REMAINDER;
            }
    }
    return KZG_OK;
}

int kzg_recover_cells_and_proofs(kzg_ctx* ctx, size_t n, unsigned log_domain, unsigned log_cell, const uint32_t* cell_ids,
                                 size_t k, const uint64_t* cells, size_t batch, uint64_t* out_coeffs, uint64_t* out_cells,
                                 uint64_t* out_proofs) {
    if (!ctx) return KZG_ERR_INVALID_ARG;
    auto invalid = [&](const std::string& why) {
        ctx->last_error = "recover: " + why;
        return KZG_ERR_INVALID_ARG;
    };
    CellsShape sh;
    if (!cells_shape(n, log_domain, log_cell, &sh)) return invalid("unsupported shape (log_domain, log_cell) or n > N");
    if (log_domain - log_cell > KZG_RECOVER_MAX_LOG_CELLS) return invalid("more than 2^KZG_RECOVER_MAX_LOG_CELLS cells");
    if (n == 0) return invalid("n = 0");
    if (k > sh.cells || k * sh.l < n) return invalid("k l must be at least n, with at most N / l cells");
    if (!cell_ids || (!cells && batch)) return invalid("a required pointer is NULL");
    std::vector<int32_t> pos(sh.cells, -1);
    for (size_t t = 0; t < k; t++) {
        if (cell_ids[t] >= sh.cells) return invalid("cell id " + std::to_string(cell_ids[t]) + " is not below N / l");
        if (pos[cell_ids[t]] >= 0) return invalid("cell id " + std::to_string(cell_ids[t]) + " appears twice");
        pos[cell_ids[t]] = (int32_t)t;
    }
    for (size_t b = 0; b < batch; b++)
        for (size_t t = 0; t < k; t++)
            for (size_t i = 0; i < sh.l; i++) {
                hf::Fr v;
                std::memcpy(v.l, cells + 4 * ((b * k + t) * sh.l + i), 32);
                if (hf::fr_geq(v, hf::kFrMod))
                    return invalid("polynomial " + std::to_string(b) + ", cell " + std::to_string(cell_ids[t]) + ": value " +
                                   std::to_string(i) + " is not below r");
            }
    if (ctx->multi) {
        int rc = KZG_OK;
        kzg_ctx* kid = cells_kid(ctx, &rc);
        return kid ? kzg_recover_cells_and_proofs(kid, n, log_domain, log_cell, cell_ids, k, cells, batch, out_coeffs, out_cells,
                                                  out_proofs)
                   : rc;
    }
    if (!batch) return KZG_OK;
    if (out_proofs) {
        std::lock_guard<std::mutex> lk(ctx->mu);
        if (!ctx->n || !ctx->slots_ready) return KZG_ERR_NO_SRS;
    }
    std::vector<uint32_t> missing;
    for (size_t j = 0; j < sh.cells; j++)
        if (pos[j] < 0) missing.push_back((uint32_t)j);
    std::vector<uint64_t> own;  // the coefficients FK20 needs when the caller does not want them
    uint64_t* coeffs = out_coeffs;
    if (!coeffs && out_proofs) {
        own.resize(batch * n * 4);
        coeffs = own.data();
    }
    const int rc = recover_host(ctx, sh, n, pos.data(), missing, k, cells, batch, coeffs, out_cells);
    if (rc || !out_proofs) return rc;
    return fk20_host(ctx, coeffs, n, batch, n, sh, nullptr, out_proofs);
}

// ---- batch verification of cell proofs (verify_kernels.hip) --------------------------------------
// One random linear combination of all records: the device forms both G1 sides, the host pairs them once.  The call holds
// fk20_mu (it reads the split twiddles glv), then the context's mutex and one slot for its stream, dropping the mutex
// while it waits for the device.
namespace {
enum : int {
    kVcCells = 0, kVcFrA, kVcFrB, kVcCoefA, kVcOrder, kVcRho, kVcIds, kVcStarts, kVcP1, kVcAff, kVcPrefix, kVcSrc, kVcGlv,
    kVcGlvSrs, kVcG1, kVcScratch, kVcWire
};
static_assert(kVcWire < 17, "kzg_ctx::vc_ws");
// the error words of one call, behind the l coefficients in the kVcCoefA workspace: the ladder's two (a point off the curve,
// outside G1), then one per class of wire input (section 4.12): proofs, commitments, values
enum : int { kVcErrCurve = 0, kVcErrG1, kVcErrWireProof, kVcErrWireCommitment, kVcErrWireValue, kVcErrWords = 8 };
constexpr uint32_t kVcFold = 16;  // terms one lane adds per level of a segmented sum, at most
// levels of a segmented sum over consecutive segments of the given lengths (each >= 1): per level the start of every
// group of at most kVcFold entries inside one segment, plus the end; stops when every segment is one entry (one level at
// least, so the result always lands in the level's output)
using VcPlan = std::vector<std::vector<uint32_t>>;
void vc_plan(std::vector<uint32_t> lens, VcPlan* levels) {
    levels->clear();
    for (;;) {
        std::vector<uint32_t> starts{0};
        bool more = false;
        for (uint32_t& len : lens) {
            const uint32_t groups = (len + kVcFold - 1) / kVcFold;
            for (uint32_t g = 0; g < groups; g++) starts.push_back(starts.back() + std::min(kVcFold, len - g * kVcFold));
            len = groups;
            more |= groups > 1;
        }
        levels->push_back(std::move(starts));
        if (!more) return;
    }
}
// uniform random bytes from the OS CSPRNG (getrandom(2)); false if it fails
bool vc_random(void* out, size_t bytes) {
    uint8_t* p = (uint8_t*)out;
    while (bytes) {
        const ssize_t got = getrandom(p, bytes, 0);
        if (got < 0) {
            if (errno == EINTR) continue;
            return false;
        }
        p += got;
        bytes -= (size_t)got;
    }
    return true;
}
const hf::Fr kFrR2 = {{0xc999e990f3f29c6dULL, 0x2b6cedcb87925c23ULL, 0x05d314967254398fULL, 0x0748d9d99f59ff11ULL}};  // 2^512 mod r
}  // namespace

namespace {
// the validated records of one call, sorted by cell id
struct VcBatch {
    const CellsShape* sh;
    size_t k, B;
    const uint64_t* commitments;
    const uint64_t* cells;
    const uint64_t* proofs;
    std::vector<uint32_t> order;  // record at sorted position t'
    std::vector<uint32_t> ids;    // the D distinct cell ids, ascending
    std::vector<uint32_t> lens;   // records per distinct id
    std::vector<Glv> glv;         // per record (input order): its weight as k1 + k2 lambda
    std::vector<Fr30> rho30;      // per sorted position: the weight in multiplier form
    std::vector<hf::Fr> U;        // per commitment: the sum of its records' weights (Montgomery)
    // openings at arbitrary points (kzg_verify_openings_batch) run the same plan with l = 1: the
    // records are grouped by distinct point, ids = 0 .. D - 1, and [z_d] T_d reads points[d], the split z_d, where the cells
    // read the context's split twiddles
    std::vector<Glv> points;
    const uint32_t* d_values = nullptr;  // the values are on the device already (in the kVcCells workspace): no upload
    bool fk20_held = false;              // the caller holds ctx->fk20_mu
    const char* what = "verify cells";
    // inputs as wire bytes (section 4.12), decoded on the device in place of the uploads of proofs / commitments / cells:
    // 48-byte compressed points (both or neither), k x l 32-byte big-endian values, every row of l in bit-reversed order or not
    const uint8_t* wire_commitments = nullptr;
    const uint8_t* wire_proofs = nullptr;
    const uint8_t* wire_values = nullptr;
    bool bit_reversed = false;
};
// the same arguments as the entry points see them; null members: that input comes decoded, as the siblings take it
struct VcWire {
    const uint8_t* commitments48 = nullptr;
    const uint8_t* proofs48 = nullptr;
    const uint8_t* values_be = nullptr;
    const uint8_t* zs_be = nullptr;
    unsigned order = KZG_ORDER_NATURAL;
};
// a 32-byte big-endian scalar on the host: false when it is not below r; out: its blst_fr image
bool wire_fr_host(const uint8_t* be, uint64_t out[4]) {
    hf::Fr v;
    for (int i = 0; i < 4; i++) {
        uint64_t w = 0;
        for (int j = 0; j < 8; j++) w = (w << 8) | be[8 * (3 - i) + j];
        v.l[i] = w;
    }
    if (hf::fr_geq(v, hf::kFrMod)) return false;
    const hf::Fr m = hf::fr_mul(v, kFrR2);
    std::memcpy(out, m.l, 32);
    return true;
}
// ... and back: the big-endian bytes of a blst_fr image
void wire_fr_to_be(const uint64_t mont[4], uint8_t out[32]) {
    hf::Fr m;
    std::memcpy(m.l, mont, 32);
    const hf::Fr one_raw = {{1, 0, 0, 0}};
    const hf::Fr v = hf::fr_mul(m, one_raw);
    for (int i = 0; i < 4; i++)
        for (int j = 0; j < 8; j++) out[8 * (3 - i) + j] = (uint8_t)(v.l[i] >> (8 * (7 - j)));
}
}  // namespace

// the two sides of the check, normalised blst_p1, into out_lhs / out_rhs
static int vc_device(kzg_ctx* ctx, const VcBatch& vb, uint64_t out_lhs[18], uint64_t out_rhs[18]) {
    const CellsShape& sh = *vb.sh;
    const size_t K = vb.k, B = vb.B, l = sh.l, D = vb.ids.size();
    const uint32_t log_M = sh.log_n - sh.log_l;
    const bool pts = !vb.points.empty();
    const std::string what = vb.what;
    // fk20_mu guards the workspaces (and glv).  kzg_verify_evaluations_batch takes it itself, before it puts the values into
    // the kVcCells workspace, and keeps it until this call returns: then vb.fk20_held is set and it is not taken again here.
    std::unique_lock<std::mutex> lkf(ctx->fk20_mu, std::defer_lock);
    if (!vb.fk20_held) lkf.lock();
    std::unique_lock<std::mutex> lk(ctx->mu);
    if (!ctx->n || !ctx->slots_ready || ctx->n < l) {
        ctx->last_error = what + (pts ? ": the SRS is empty" : ": the SRS holds fewer than l points");
        return KZG_ERR_NO_SRS;
    }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    int rc = pts ? KZG_OK : ensure_ntt(ctx);
    if (rc) return rc;
    const int slot = reserve_slot(ctx, lk, true);
    if (slot < 0) return KZG_ERR_BUSY;
    SlotLease lease{ctx, slot};
    Slot& s = ctx->slots[slot];
    rc = ensure_slot_basics(ctx, s);
    if (rc == KZG_OK && !pts) rc = ensure_glv(ctx, lk, log_M, s.stream);
    if (rc) return rc;
    // plans: T_j by cell id; the column sums of the twisted rows (one segment of D); the two sides over [T | C | S | AT]
    VcPlan plan_t, plan_col, plan_fin;
    vc_plan(vb.lens, &plan_t);
    vc_plan({(uint32_t)D}, &plan_col);
    vc_plan({(uint32_t)D, (uint32_t)(B + l + D)}, &plan_fin);
    std::vector<uint32_t> starts;
    std::vector<size_t> at_t, at_col, at_fin;  // offsets of each level's starts in the upload
    for (auto* pl : {&plan_t, &plan_col, &plan_fin}) {
        auto& at = pl == &plan_t ? at_t : (pl == &plan_col ? at_col : at_fin);
        for (const auto& lv : *pl) {
            at.push_back(starts.size());
            starts.insert(starts.end(), lv.begin(), lv.end());
        }
    }
    const size_t g0 = plan_t[0].size() - 1;  // rows after the first level (>= D)
    const size_t gmax = std::max(g0, plan_fin[0].size() - 1);
    const size_t lanes = K + B;
    std::vector<uint32_t> src(lanes);
    std::vector<Glv> glv(lanes);
    for (size_t t = 0; t < K; t++) {
        src[t] = vb.order[t];
        glv[t] = vb.glv[vb.order[t]];
    }
    for (size_t b = 0; b < B; b++) {
        src[K + b] = (uint32_t)(K + b);
        glv[K + b] = glv_split(vb.U[b]);
    }
    void *cells, *fa, *fb, *coef, *order, *rho, *ids, *dstarts, *p1, *aff, *prefix, *dsrc, *dglv, *dglvs, *g1, *scratch;
    void* wire = nullptr;  // the values' bytes (the points' go through the p1 workspace, which is free until the sides land in it)
    // values already on the device ARE the kVcCells workspace: asking for it again could free and reallocate it (vc_ws drops
    // the contents when it grows)
    if (vb.d_values) cells = (void*)vb.d_values;
    else rc = ctx->vc_ws.get(ctx, kVcCells, K * l * 32, &cells);
    if (rc == KZG_OK) rc = ctx->vc_ws.get(ctx, kVcFrA, g0 * l * 32, &fa);
    if (rc == KZG_OK) rc = ctx->vc_ws.get(ctx, kVcFrB, g0 * l * 32, &fb);
    if (rc == KZG_OK && vb.wire_values) rc = ctx->vc_ws.get(ctx, kVcWire, K * l * 32, &wire);
    if (rc == KZG_OK) rc = ctx->vc_ws.get(ctx, kVcCoefA, l * 32 + kVcErrWords * 4, &coef);  // + the error words
    if (rc == KZG_OK) rc = ctx->vc_ws.get(ctx, kVcOrder, K * 4, &order);
    if (rc == KZG_OK) rc = ctx->vc_ws.get(ctx, kVcRho, K * sizeof(Fr30), &rho);
    if (rc == KZG_OK) rc = ctx->vc_ws.get(ctx, kVcIds, D * 4, &ids);
    if (rc == KZG_OK) rc = ctx->vc_ws.get(ctx, kVcStarts, starts.size() * 4, &dstarts);
    if (rc == KZG_OK) rc = ctx->vc_ws.get(ctx, kVcP1, lanes * 144, &p1);
    if (rc == KZG_OK) rc = ctx->vc_ws.get(ctx, kVcAff, lanes * kAffineBytes, &aff);
    if (rc == KZG_OK) rc = ctx->vc_ws.get(ctx, kVcPrefix, lanes * 64, &prefix);
    if (rc == KZG_OK) rc = ctx->vc_ws.get(ctx, kVcSrc, lanes * 4, &dsrc);
    if (rc == KZG_OK) rc = ctx->vc_ws.get(ctx, kVcGlv, lanes * sizeof(Glv), &dglv);
    if (rc == KZG_OK) rc = ctx->vc_ws.get(ctx, kVcGlvSrs, (l + vb.points.size()) * sizeof(Glv), &dglvs);  // then the split points
    if (rc == KZG_OK) rc = ctx->vc_ws.get(ctx, kVcG1, (K + 2 * D + B + l + 2) * kXyzzBytes, &g1);
    if (rc == KZG_OK) rc = ctx->vc_ws.get(ctx, kVcScratch, 2 * gmax * kXyzzBytes, &scratch);
    if (rc) return rc;
    const hipStream_t st = s.stream;
    uint32_t* err = (uint32_t*)((char*)coef + l * 32);
    HIP_TRY(ctx, hipMemsetAsync(err, 0xff, kVcErrWords * 4, st));
    if (vb.wire_values) {
        HIP_TRY(ctx, hipMemcpyAsync(wire, vb.wire_values, K * l * 32, hipMemcpyHostToDevice, st));
        launch_wire_fr(st, wire, (uint32_t)(K * l), sh.log_l, vb.bit_reversed, cells, err + kVcErrWireValue);
    } else if (!vb.d_values) {
        HIP_TRY(ctx, hipMemcpyAsync(cells, vb.cells, K * l * 32, hipMemcpyHostToDevice, st));
    }
    Glv* dpoints = (Glv*)dglvs + l;
    if (pts) HIP_TRY(ctx, hipMemcpyAsync(dpoints, vb.points.data(), D * sizeof(Glv), hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipMemcpyAsync(order, vb.order.data(), K * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipMemcpyAsync(rho, vb.rho30.data(), K * sizeof(Fr30), hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipMemcpyAsync(ids, vb.ids.data(), D * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipMemcpyAsync(dstarts, starts.data(), starts.size() * 4, hipMemcpyHostToDevice, st));
    if (vb.wire_proofs) {
        HIP_TRY(ctx, hipMemcpyAsync(p1, vb.wire_proofs, K * 48, hipMemcpyHostToDevice, st));
        if (B) HIP_TRY(ctx, hipMemcpyAsync((char*)p1 + K * 48, vb.wire_commitments, B * 48, hipMemcpyHostToDevice, st));
    } else {
        HIP_TRY(ctx, hipMemcpyAsync(p1, vb.proofs, K * 144, hipMemcpyHostToDevice, st));
        if (B) HIP_TRY(ctx, hipMemcpyAsync((char*)p1 + K * 144, vb.commitments, B * 144, hipMemcpyHostToDevice, st));
    }
    HIP_TRY(ctx, hipMemcpyAsync(dsrc, src.data(), lanes * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipMemcpyAsync(dglv, glv.data(), lanes * sizeof(Glv), hipMemcpyHostToDevice, st));
    const uint32_t* dst_ = (const uint32_t*)dstarts;
    // Fr side: V_j (weighted first level), the inverse transforms, the twist, the column sums -> A's l coefficients
    uint32_t *FA = (uint32_t*)fa, *FB = (uint32_t*)fb;
    const uint32_t* cur = (const uint32_t*)cells;
    for (size_t lv = 0; lv < plan_t.size(); lv++) {
        uint32_t* dst = cur == FA ? FB : FA;
        launch_vc_fr_sum(st, cur, lv ? nullptr : (const uint32_t*)order, lv ? nullptr : (const Fr30*)rho, dst_ + at_t[lv],
                         (uint32_t)(plan_t[lv].size() - 1), sh.log_l, dst);
        cur = dst;
    }
    const Fr30* tw = (const Fr30*)ctx->ntt_tw.p;
    if (!pts) {  // (a point's "interpolant" is its value: nothing to transform)
        uint32_t* y = const_cast<uint32_t*>(launch_fr_dft(st, cur, FA, FB, sh.log_l, D, tw + 2 * kNttTableLen));
        launch_vc_fr_twist(st, y, (const uint32_t*)ids, (uint32_t)D, tw + 2 * kNttTableLen, sh.log_n, sh.log_l,
                           fr30_arg_from_mont256(hf::fr_inv(fr_pow2(sh.log_l))));
        cur = y;
    }
    for (size_t lv = 0; lv < plan_col.size(); lv++) {
        uint32_t* dst = lv + 1 == plan_col.size() ? (uint32_t*)coef : (cur == FA ? FB : FA);
        launch_vc_fr_sum(st, cur, nullptr, nullptr, dst_ + at_col[lv], (uint32_t)(plan_col[lv].size() - 1), sh.log_l, dst);
        cur = dst;
    }
    // G1: [P: K | T: D | C: B | S: l | AT: D | the two sides]
    const size_t oT = K, oC = K + D, oS = oC + B, oAT = oS + l, oOut = oAT + D;
    auto rec = [&](size_t i) { return (void*)((char*)g1 + i * kXyzzBytes); };
    void* X[2] = {scratch, (char*)scratch + gmax * kXyzzBytes};
    if (vb.wire_proofs) {  // straight into the records the ladder reads, in input order: no normalisation to run
        launch_wire_g1(st, p1, nullptr, (uint32_t)K, aff, (uint32_t)kAffineBytes, err + kVcErrWireProof);
        launch_wire_g1(st, (char*)p1 + K * 48, nullptr, (uint32_t)B, (char*)aff + K * kAffineBytes, (uint32_t)kAffineBytes,
                       err + kVcErrWireCommitment);
    } else {
        launch_jacobian_to_affine(st, p1, (uint32_t)lanes, aff, prefix);
    }
    launch_vc_ladder(st, aff, (const uint32_t*)dsrc, (const Glv*)dglv, (uint32_t)lanes, (uint32_t)lanes, (uint32_t)K, rec(0), rec(oC),
                     err);
    auto g1_plan = [&](const VcPlan& plan, const std::vector<size_t>& at, const void* in, void* out) {
        const void* c = in;
        for (size_t lv = 0; lv < plan.size(); lv++) {
            void* dst = lv + 1 == plan.size() ? out : (c == X[0] ? X[1] : X[0]);
            launch_vc_g1_sum(st, c, dst_ + at[lv], (uint32_t)(plan[lv].size() - 1), dst);
            c = dst;
        }
    };
    g1_plan(plan_t, at_t, rec(0), rec(oT));
    if (pts) launch_vc_cell_scale(st, rec(oT), (const uint32_t*)ids, (uint32_t)D, dpoints, 0, rec(oAT));
    else launch_vc_cell_scale(st, rec(oT), (const uint32_t*)ids, (uint32_t)D, (const Glv*)ctx->glv.p, ctx->glv_log - log_M, rec(oAT));
    HIP_TRY(ctx, hipGetLastError());
    rc = sync_unlocked(ctx, lk, st, what.c_str());
    if (rc) return rc;
    std::vector<hf::Fr> A(l);
    uint32_t herr[kVcErrWords];
    HIP_TRY(ctx, hipMemcpyAsync(A.data(), coef, l * 32, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipMemcpyAsync(herr, err, sizeof herr, hipMemcpyDeviceToHost, st));
    rc = sync_unlocked(ctx, lk, st, "verify cells");
    if (rc) return rc;
    if (herr[kVcErrWireProof] != 0xffffffffu || herr[kVcErrWireCommitment] != 0xffffffffu) {
        const bool proof = herr[kVcErrWireProof] != 0xffffffffu;
        ctx->last_error = what + ": " + (proof ? "the proof of record " + std::to_string(herr[kVcErrWireProof])
                                               : "commitment " + std::to_string(herr[kVcErrWireCommitment])) +
                          " is not a valid compressed point";
        return KZG_ERR_INVALID_ARG;
    }
    if (herr[kVcErrWireValue] != 0xffffffffu) {
        const uint32_t g = herr[kVcErrWireValue];
        ctx->last_error = what + ": record " + std::to_string(g >> sh.log_l) +
                          (pts ? ": the claimed y" : ": value " + std::to_string(g & (l - 1))) + " is not below r";
        return KZG_ERR_INVALID_ARG;
    }
    for (int e = 0; e < 2; e++)
        if (herr[e] != 0xffffffffu) {
            const std::string who = herr[e] < K ? "the proof of record " + std::to_string(herr[e])
                                                 : "commitment " + std::to_string(herr[e] - K);
            ctx->last_error = what + ": " + who + (e ? " is not in G1" : " is not on the curve");
            return KZG_ERR_INVALID_ARG;
        }
    // -[A(s)]G1 = sum_i [-A_i] [s^i]G1
    std::vector<Glv> gs(l);
    const hf::Fr zero = {{0, 0, 0, 0}};
    for (size_t i = 0; i < l; i++) gs[i] = glv_split(hf::fr_sub(zero, A[i]));
    HIP_TRY(ctx, hipMemcpyAsync(dglvs, gs.data(), l * sizeof(Glv), hipMemcpyHostToDevice, st));
    launch_vc_ladder(st, ctx->table.p, nullptr, (const Glv*)dglvs, (uint32_t)l, 0, 0, nullptr, rec(oS), err);
    g1_plan(plan_fin, at_fin, rec(oT), rec(oOut));
    launch_xyzz_to_affine(st, rec(oOut), 2, aff, prefix);
    launch_affine_to_p1(st, aff, 2, p1);
    HIP_TRY(ctx, hipGetLastError());
    rc = sync_unlocked(ctx, lk, st, "verify cells");  // gs goes out of scope
    if (rc) return rc;
    uint64_t sides[36];
    HIP_TRY(ctx, hipMemcpyAsync(sides, p1, 2 * 144, hipMemcpyDeviceToHost, st));
    rc = sync_unlocked(ctx, lk, st, "verify cells");
    if (rc) return rc;
    std::memcpy(out_lhs, sides, 144);
    std::memcpy(out_rhs, sides + 18, 144);
    return KZG_OK;
}

// G1 inputs: canonical coordinates, and not the all-zero affine image of a finite point (the device's infinity); the curve
// and subgroup checks run on the device
static bool vc_p1_malformed(const uint64_t* w) {
    hf::P1 p;
    std::memcpy(&p, w, sizeof p);
    if (!hf::geq(p.x, hf::kP) && !hf::geq(p.y, hf::kP) && !hf::geq(p.z, hf::kP))
        return !p.z.is_zero() && p.x.is_zero() && p.y.is_zero();
    return true;
}
// the weights of k records: rho = a + b lambda with a, b uniform 64-bit from the OS CSPRNG (a plain integer below 2^193 < r),
// or the caller's (validated below r); rho in Montgomery form, glv its split
static int vc_weights(kzg_ctx* ctx, const char* what, const uint64_t* weights, size_t k, std::vector<hf::Fr>* rho,
                      std::vector<Glv>* glv) {
    rho->resize(k);
    glv->resize(k);
    if (weights) {
        for (size_t t = 0; t < k; t++) {
            std::memcpy((*rho)[t].l, weights + 4 * t, 32);
            (*glv)[t] = glv_split((*rho)[t]);
        }
        return KZG_OK;
    }
    std::vector<uint64_t> ab(2 * k);
    if (!vc_random(ab.data(), ab.size() * 8)) {
        ctx->last_error = std::string(what) + ": getrandom: " + std::strerror(errno);
        return KZG_ERR_HIP;
    }
    for (size_t t = 0; t < k; t++) {
        const uint64_t a = ab[2 * t], b = ab[2 * t + 1];
        const unsigned __int128 lo = (unsigned __int128)b * (uint64_t)kGlvLambda + a;
        const unsigned __int128 hi = (unsigned __int128)b * (uint64_t)(kGlvLambda >> 64) + (uint64_t)(lo >> 64);
        const hf::Fr raw = {{(uint64_t)lo, (uint64_t)hi, (uint64_t)(hi >> 64), 0}};
        (*rho)[t] = hf::fr_mul(raw, kFrR2);  // Montgomery
        (*glv)[t] = Glv{{a, 0}, {b, 0}};
    }
    return KZG_OK;
}
// e(LHS, Q) == e(RHS, G2):  e(LHS, Q) e(-RHS, G2) == 1
static int vc_pair(const uint64_t lhs[18], const uint64_t rhs[18], const hf::G2Affine& q, const hf::G2Affine& g2_one) {
    hf::P1 L, R;
    std::memcpy(&L, lhs, sizeof L);
    std::memcpy(&R, rhs, sizeof R);
    const hf::G2Affine qs[2] = {q, g2_one};
    const hf::P1 ps[2] = {L, hf::p1_neg(R)};
    bool ok = true;
    const hf::F12 f = hf::multi_miller_loop(qs, ps, 2, ok);
    return ok && hf::f12_is_one(hf::f12_final_exp(f)) ? 1 : 0;
}

// what the two verifiers check alike on the host: the caller's weights below r (weights null: random ones will be drawn), the
// G1 inputs well formed, setup_g2[0] and setup_g2[second] on the twist (into g2[0], g2[1]); second_name: how the error text
// calls that index
static int vc_check_inputs(kzg_ctx* ctx, const char* what, const uint64_t* weights, const uint64_t* proofs_p1, size_t k,
                           const uint64_t* commitments_p1, size_t num_commitments, const void* setup_g2, size_t g2_stride_bytes,
                           size_t second, const char* second_name, hf::G2Affine g2[2], bool wire_points = false) {
    auto invalid = [&](const std::string& why) {
        ctx->last_error = std::string(what) + ": " + why;
        return KZG_ERR_INVALID_ARG;
    };
    if (weights)
        for (size_t t = 0; t < k; t++) {
            hf::Fr v;
            std::memcpy(v.l, weights + 4 * t, 32);
            if (hf::fr_geq(v, hf::kFrMod)) return invalid("weight " + std::to_string(t) + " is not below r");
        }
    for (size_t t = 0; t < k && !wire_points; t++)  // (compressed points: the device's decoder checks them)
        if (vc_p1_malformed(proofs_p1 + 18 * t)) return invalid("the proof of record " + std::to_string(t) + " is not on the curve");
    for (size_t b = 0; b < num_commitments && !wire_points; b++)
        if (vc_p1_malformed(commitments_p1 + 18 * b)) return invalid("commitment " + std::to_string(b) + " is not on the curve");
    for (int i = 0; i < 2; i++) {
        uint64_t raw[36];
        std::memcpy(raw, (const uint8_t*)setup_g2 + (i ? second : 0) * g2_stride_bytes, sizeof raw);
        g2[i] = hf::g2_from_p2(raw);
        if (!hf::g2_on_curve(g2[i])) return invalid(std::string("setup_g2[") + (i ? second_name : "0") + "] is not on the twist");
    }
    return KZG_OK;
}

// a call forwarded to a device's context before its inputs were checked: the parent reports what that context found
static int forwarded(kzg_ctx* ctx, kzg_ctx* kid, int rc) {
    if (rc) ctx->last_error = kid->last_error;
    return rc;
}
// The device a prover call on a multi-device context is forwarded to.  Without commitments (`wanted` false) the call needs no SRS;
// with them it follows kzg_commit_lagrange: a replicated context forwards, a range-split one holds no whole SRS on one device and
// refuses (null: KZG_ERR_INVALID_ARG, the message begins with `what_needs`)
static kzg_ctx* whole_srs_kid(kzg_ctx* ctx, bool wanted, const char* what_needs) {
    if (wanted && multi_mode(ctx->multi) != kMultiReplicate) {
        ctx->last_error = std::string(what_needs) + " the whole SRS on one device: not on a range-split multi-device context";
        return nullptr;
    }
    return multi_kid(ctx->multi, 0);
}

// ---- the quotient of a permutation argument on the coset g H_N (quotient_kernels.hip) ---------------------
// Every call holds quotient_mu, then the context's mutex and one slot for its stream, dropping the mutex while it copies or waits
// (PqCall, below).
namespace {
enum : int { kPqIn = 0, kPqCols, kPqT, kPqP, kPqA, kPqB, kPqOut, kPqCoef, kPqGate, kPqZinv, kPqFlag, kPqBlind, kPqChunks, kPqCount };
constexpr size_t kPqMaxChunk = 64;                 // the transform buffers of one pass (ctx->pq_ws_budget) hold at most this many columns
constexpr uint32_t kPqDftLog = kNttTileLog;        // below 2^11 values a batch takes launch_fr_dft, from there on launch_ntt per column
static_assert(kPqCount <= 13, "pq_ws");

// waits for what a call left on its slot's streams (no slot yet: nothing)
struct PqDrain {
    const Slot* s = nullptr;  // the front stream, and the stream a commitment of the chunks ended on
    void now() const {
        if (s && s->stream) (void)hipStreamSynchronize(s->stream);
        if (s && s->end && s->end != s->stream) (void)hipStreamSynchronize(s->end);
    }
    ~PqDrain() { now(); }
};

struct PqShape {
    uint32_t lg_n = 0, lg_ext = 0, lg_N = 0;
    size_t n = 0, rot = 0, N = 0;
};
// n = 2^k, rot = 2^x with x <= 3, N = rot n <= 2^22
bool pq_shape(size_t n, size_t rot, PqShape* sh) {
    uint32_t a = 0, b = 0;
    if (!ntt_log(n, &a) || !ntt_log(rot, &b) || b > kPqMaxLogExt || a + b > kNttMaxLog) return false;
    *sh = PqShape{a, b, a + b, n, rot, n * rot};
    return true;
}
Fr30 pq_image(const hf::Fr& v) {
    uint32_t l[8];
    std::memcpy(l, v.l, 32);
    return fr30_from_limbs(l);
}
hf::Fr pq_fr(const uint64_t* p) {
    hf::Fr v;
    std::memcpy(v.l, p, 32);
    return v;
}
bool pq_overlap(const void* a, size_t a_bytes, const void* b, size_t b_bytes) {
    return (const char*)a < (const char*)b + b_bytes && (const char*)b < (const char*)a + a_bytes;
}

// the transform buffers of one pass: `chunk` columns of N values each
struct PqBufs {
    uint32_t *T = nullptr, *P = nullptr, *A = nullptr, *B = nullptr;
    size_t chunk = 0;
};
// ctx->mu held, the caller has waited for every earlier use of the workspaces
int pq_bufs(kzg_ctx* ctx, size_t N, size_t cols, PqBufs* w) {
    size_t chunk = ctx->pq_ws_budget / (4 * N * 32);
    chunk = chunk < 1 ? 1 : (chunk > kPqMaxChunk ? kPqMaxChunk : chunk);
    if (chunk > cols) chunk = cols ? cols : 1;
    void *t, *p, *a, *b;
    int rc = ctx->pq_ws.get(ctx, kPqT, chunk * N * 32, &t);
    if (rc == KZG_OK) rc = ctx->pq_ws.get(ctx, kPqP, chunk * N * 32, &p);
    if (rc == KZG_OK) rc = ctx->pq_ws.get(ctx, kPqA, chunk * N * 32, &a);
    if (rc == KZG_OK) rc = ctx->pq_ws.get(ctx, kPqB, chunk * N * 32, &b);
    *w = PqBufs{(uint32_t*)t, (uint32_t*)p, (uint32_t*)a, (uint32_t*)b, chunk};
    return rc;
}

// A round of kzg_circuit_prove inside one of the circuit calls' bodies: the caller holds quotient_mu, the context's mutex (*lk) and
// the slot, has raised the batched pass kernel's LDS limit, and keeps the UNBLINDED coefficients of the per-proof columns resident,
// n each, back to back: [ f_0 .. f_(t-1) | PI (when the call is given public inputs) | z ].  The body then takes no lock and no
// slot, transforms no column back (it reads `coef`; its wires / z / PI arguments only say what is there) and extends several
// columns with launch_ntt_batch.
struct ProveRound {
    std::unique_lock<std::mutex>* lk = nullptr;
    int slot = -1;
    const uint32_t* coef = nullptr;
    // the opening: v from the 2 t evaluations, once they are known (false: refused)
    std::function<bool(const uint64_t* evals, uint64_t v[4])> derive_v;
};

// `cols` columns (column j: len entries at src + 8 j stride words; src null: every entry is *fill) onto the coset of N = 2^lg_N
// points, column j to dst + 8 j N words.  lg_len >= 0: the entries are values over the domain of 2^lg_len points (inverse
// transform, twist by g^i / len, padding, forward transform); lg_len < 0: they are coefficients (twist, padding, forward
// transform).  dst overlaps neither src nor the buffers.
int pq_extend(kzg_ctx* ctx, hipStream_t st, const uint32_t* src, size_t stride, size_t len, int lg_len, size_t cols, uint32_t lg_N,
              uint32_t* dst, const PqBufs& w, const Fr30* fill = nullptr, bool batched = false) {
    const size_t N = (size_t)1 << lg_N;
    const Fr30* tw = (const Fr30*)ctx->ntt_tw.p;
    const Fr30* itw = tw + 2 * kNttTableLen;
    const Fr30* gt = (const Fr30*)ctx->rec_g.p;
    const Fr30 one = fr30_arg_from_mont256(hf::kFrOne);
    for (size_t c0 = 0; c0 < cols; c0 += w.chunk) {
        const size_t bc = cols - c0 < w.chunk ? cols - c0 : w.chunk;
        const uint32_t* coef = src ? src + 8 * c0 * stride : nullptr;
        size_t cstride = stride;
        Fr30 c = one;
        if (lg_len >= 0) {
            const Fr30 inv_len = fr30_arg_from_mont256(hf::fr_inv(fr_pow2((uint32_t)lg_len)));
            if ((uint32_t)lg_len >= kPqDftLog) {  // the last pass multiplies by 1 / len
                for (size_t b = 0; b < bc; b++)
                    launch_ntt(st, coef + 8 * b * stride, w.T + 8 * b * len, (uint32_t)lg_len, itw, inv_len, w.A, w.B);
                coef = w.T;
            } else {  // one batch of contiguous vectors, unnormalised
                if (stride != len && bc > 1) {
                    HIP_TRY(ctx, hipMemcpy2DAsync(w.T, len * 32, coef, stride * 32, len * 32, bc, hipMemcpyDeviceToDevice, st));
                    coef = w.T;
                }
                coef = launch_fr_dft(st, coef, w.A, w.B, (uint32_t)lg_len, bc, itw);
                c = inv_len;
            }
            cstride = len;
        }
        launch_pq_pad_twist(st, coef, cstride, (uint32_t)len, fill ? *fill : one, lg_N, bc, gt, c, w.P);
        if (lg_N >= kPqDftLog && batched && bc > 1) {  // (kzg_circuit_prove: one launch per pass for the chunk's columns)
            launch_ntt_batch(st, w.P, N, dst + 8 * c0 * N, N, lg_N, (uint32_t)bc, tw, one, w.A, w.B);
        } else if (lg_N >= kPqDftLog) {
            for (size_t b = 0; b < bc; b++) launch_ntt(st, w.P + 8 * b * N, dst + 8 * (c0 + b) * N, lg_N, tw, one, w.A, w.B);
        } else {
            const uint32_t* ev = launch_fr_dft(st, w.P, w.A, w.B, lg_N, bc, tw);
            HIP_TRY(ctx, hipMemcpyAsync(dst + 8 * c0 * N, ev, bc * N * 32, hipMemcpyDeviceToDevice, st));
        }
        HIP_TRY(ctx, hipGetLastError());
    }
    return KZG_OK;
}

// the rot stored multipliers 1 / Z_H(x_i), Z_H(x_i) = g^n w_rot^(i mod rot) - 1 (never zero: 7 has order r - 1), on the device.
// They depend on (n, rot) only: the table of the last shape stays (pq_zinv_key), so that a repeated shape costs neither the rot
// host inversions nor the upload and the wait for it.
int pq_upload_zinv(kzg_ctx* ctx, std::unique_lock<std::mutex>& lk, hipStream_t st, const PqShape& sh, uint32_t** d_zinv) {
    void* d = nullptr;
    int rc = ctx->pq_ws.get(ctx, kPqZinv, 8 * 32, &d);
    if (rc) return rc;
    *d_zinv = (uint32_t*)d;
    const uint32_t key = (sh.lg_n << 8) | sh.lg_ext;
    if (ctx->pq_zinv_key == key) return KZG_OK;
    ctx->pq_zinv_key = ~0u;
    uint64_t h[8][4];
    const hf::Fr we = hf::fr_domain_root(sh.lg_ext), k14 = fr_pow2(14);
    hf::Fr cur = hf::fr_pow(fr_seven(), sh.n);
    for (size_t k = 0; k < sh.rot; k++) {
        const hf::Fr stored = hf::fr_mul(hf::fr_inv(hf::fr_sub(cur, hf::kFrOne)), k14);  // the x 2^270 form, canonical
        std::memcpy(h[k], stored.l, 32);
        cur = hf::fr_mul(cur, we);
    }
    rc = copy_unlocked(ctx, lk, st, d, h, sh.rot * 32, hipMemcpyHostToDevice, "hipMemcpyAsync (vanishing inverses)");
    if (rc == KZG_OK) rc = sync_unlocked(ctx, lk, st, "quotient");  // (h leaves scope)
    if (rc == KZG_OK) ctx->pq_zinv_key = key;
    return rc;
}

struct PqChallenges {
    const uint64_t *shifts, *alpha, *beta, *gamma;
};
// The challenges as the constraint kernels take them (engine.h, PqScalars), for t columns: beta, alpha 2^(14 t) and alpha^2 2^14
// in multiplier form; gamma, one and beta k_j g as the digits of their images; k14 = 2^14 in multiplier form (the circuit kernel).
// The kernels' bound comments and test_fr_extremes* rest on these magnitudes: they are made here and nowhere else.
struct PqKernelScalars {
    Fr30 beta, gamma, one, a1, a2, k14, bkg[kPqMaxColumns];
    PqKernelScalars(const PqChallenges& ch, size_t t) {
        const hf::Fr a = pq_fr(ch.alpha), b = pq_fr(ch.beta), g = fr_seven();
        beta = fr30_arg_from_mont256(b);
        gamma = pq_image(pq_fr(ch.gamma));
        one = pq_image(hf::kFrOne);
        a1 = fr30_arg_from_mont256(hf::fr_mul(a, fr_pow2((uint32_t)(14 * t))));
        a2 = fr30_arg_from_mont256(hf::fr_mul(hf::fr_mul(a, a), fr_pow2(14)));
        k14 = fr30_arg_from_mont256(fr_pow2(14));
        for (size_t j = 0; j < t; j++) bkg[j] = pq_image(hf::fr_mul(hf::fr_mul(b, pq_fr(ch.shifts + 4 * j)), g));
    }
    PqScalars view() const { return PqScalars{&beta, &gamma, &one, &a1, &a2, bkg}; }
};
// Num / Z_H on the coset into d_out (N values): the extended columns at d_wires / d_sigmas (column j at + 8 j stride words), d_z,
// d_gate (or null); the values of L_0 are made in d_l0 here
int pq_constraints(kzg_ctx* ctx, std::unique_lock<std::mutex>& lk, hipStream_t st, const PqShape& sh, size_t t, size_t stride,
                   const uint32_t* d_wires, const uint32_t* d_sigmas, const uint32_t* d_z, const uint32_t* d_gate, uint32_t* d_l0,
                   const PqChallenges& ch, const PqBufs& w, uint32_t* d_out) {
    uint32_t* d_zinv = nullptr;
    int rc = pq_upload_zinv(ctx, lk, st, sh, &d_zinv);
    if (rc) return rc;
    // L_0 = (1 / n) (1 + X + .. + X^(n-1)): one more extension, from n equal coefficients
    const Fr30 inv_n = pq_image(hf::fr_inv(fr_pow2(sh.lg_n)));
    rc = pq_extend(ctx, st, nullptr, 0, sh.n, -1, 1, sh.lg_N, d_l0, w, &inv_n);
    if (rc) return rc;
    const PqKernelScalars sc(ch, t);
    const PqColumns cols{d_wires, d_sigmas, d_z, d_l0, d_gate, d_zinv};
    launch_pq_constraints(st, cols, sh.lg_N, (uint32_t)sh.rot, (uint32_t)t, stride, sc.view(), ctx->ntt_tw.p, d_out);
    HIP_TRY(ctx, hipGetLastError());
    return KZG_OK;
}
// Num / Z_H of a circuit on the coset into d_out (N values), the arithmetic gate built in: the call's extended wires (column j at
// d_w + 8 j N words), z, PI (or null) and gate (or null), and the key's columns where kzg_circuit_create laid them in c->coset:
// q_lin first, q_M at + t N, q_C at + (t + 1) N, the sigmas at + (t + 2) N
int ck_constraints(kzg_ctx* ctx, hipStream_t st, const kzg_circuit* c, const PqShape& sh, const uint32_t* d_w, const uint32_t* d_z,
                   const uint32_t* d_pi, const uint32_t* d_gate, const uint64_t* alpha, const uint64_t* beta, const uint64_t* gamma,
                   uint32_t* d_out) {
    const size_t t = c->t, N = sh.N;
    const PqKernelScalars sc(PqChallenges{c->shifts, alpha, beta, gamma}, t);
    const uint32_t* key = c->coset.dev();
    const CkColumns ck{d_w, key, key + 8 * (t + 2) * N, key + 8 * t * N, key + 8 * (t + 1) * N, d_z, c->l0.dev(), d_pi, d_gate, c->zinv.dev()};
    launch_ck_constraints(st, ck, sh.lg_N, (uint32_t)sh.rot, (uint32_t)t, N, sc.view(), sc.k14, ctx->ntt_tw.p, d_out);
    HIP_TRY(ctx, hipGetLastError());
    return KZG_OK;
}

// N values on the coset in d_vals (a workspace: divided in place unless already divided) -> the N - n coefficients of the
// quotient in d_coef; *d_flag (zeroed here) is set when a coefficient at [N - n, N) is not zero.  keep != 0 (a blinded quotient,
// whose degree passes N - n): the first `keep` coefficients are written and the flag looks at [keep, N)
int pq_interpolate(kzg_ctx* ctx, std::unique_lock<std::mutex>& lk, hipStream_t st, const PqShape& sh, uint32_t* d_vals, bool divide,
                   const PqBufs& w, uint32_t* d_coef, uint32_t* d_flag, size_t keep = 0) {
    if (!keep) keep = sh.N - sh.n;
    const Fr30* itw = (const Fr30*)ctx->ntt_tw.p + 2 * kNttTableLen;
    const Fr30* ginv = (const Fr30*)ctx->rec_g.p + 2 * kNttTableLen;
    const Fr30 one = fr30_arg_from_mont256(hf::kFrOne), inv_N = fr30_arg_from_mont256(hf::fr_inv(fr_pow2(sh.lg_N)));
    if (divide) {
        uint32_t* d_zinv = nullptr;
        int rc = pq_upload_zinv(ctx, lk, st, sh, &d_zinv);
        if (rc) return rc;
        launch_recover_divide(st, d_vals, sh.lg_N, sh.lg_n, 1, d_zinv);  // by index mod rot
    }
    HIP_TRY(ctx, hipMemsetAsync(d_flag, 0, 4, st));
    if (sh.lg_N >= kPqDftLog) {
        launch_ntt(st, d_vals, w.T, sh.lg_N, itw, inv_N, w.A, w.B);
        launch_recover_untwist(st, w.T, sh.lg_N, (uint32_t)keep, 1, ginv, one, d_coef, false, d_flag);
    } else {
        const uint32_t* cur = launch_fr_dft(st, d_vals, w.A, w.B, sh.lg_N, 1, itw);
        launch_recover_untwist(st, const_cast<uint32_t*>(cur), sh.lg_N, (uint32_t)keep, 1, ginv, inv_N, d_coef, false, d_flag);
    }
    HIP_TRY(ctx, hipGetLastError());
    return KZG_OK;
}
int pq_remainder(kzg_ctx* ctx, const PqShape& sh) {
    ctx->last_error = "quotient: the numerator is not divisible by X^" + std::to_string(sh.n) +
                      " - 1 (a coefficient of the interpolant at [N - n, N) is not zero): the constraints do not hold on the domain";
    return KZG_ERR_REMAINDER;
}

// The end of a quotient: the N values in d_vals -> coefficients in d_coef (pq_interpolate), `out_len` of them to host_out where
// that is not null, the wait under the call's name.  *remainder: the flag -- the caller words its own refusal
int pq_finish(kzg_ctx* ctx, std::unique_lock<std::mutex>& lk, hipStream_t st, const PqShape& sh, uint32_t* d_vals, bool divide,
              const PqBufs& w, uint32_t* d_coef, uint32_t* d_flag, size_t keep, size_t out_len, void* host_out, const char* what,
              bool* remainder) {
    int rc = pq_interpolate(ctx, lk, st, sh, d_vals, divide, w, d_coef, d_flag, keep);
    uint32_t hflag = 0;
    if (rc == KZG_OK) rc = copy_unlocked(ctx, lk, st, &hflag, d_flag, 4, hipMemcpyDeviceToHost, "hipMemcpyAsync (flag)");
    if (rc == KZG_OK && host_out)
        rc = copy_unlocked(ctx, lk, st, host_out, d_coef, out_len * 32, hipMemcpyDeviceToHost, "hipMemcpyAsync (quotient)");
    if (rc == KZG_OK) rc = sync_unlocked(ctx, lk, st, what);
    *remainder = hflag != 0;
    return rc;
}

// the SRS a call's commitments of `need_len` coefficients need (ctx->mu held); none where no commitment is wanted
int pq_srs_status(const kzg_ctx* ctx, bool wanted, size_t need_len) {
    if (!wanted) return KZG_OK;
    if (!ctx->n || !ctx->slots_ready) return KZG_ERR_NO_SRS;
    return need_len > ctx->n ? KZG_ERR_DEGREE_TOO_HIGH : KZG_OK;
}

int ensure_ntt_batch(kzg_ctx* ctx);
// What a call of this family holds, and the order it gives it back in.  An owning frame takes quotient_mu when it is made, the
// context's mutex in lock() and the tables and a reserved slot with its stream in begin(): three steps, because the bodies check
// their arguments and the SRS between them.  An adopted frame (a round of kzg_circuit_prove, whose caller holds all three) takes
// nothing and gives nothing back.
// The members go last to first, and that IS the order of release.  First the streams are drained, by either kind of frame:
// whatever way a call returns -- also after a failed copy or launch -- nothing it enqueued still uses pq_ws when the slot and
// quotient_mu are given up (a later call may grow, that is free, a workspace); after a call that ended well the stream is empty and
// this costs nothing.  Then the slot goes back, under the context's mutex; then that mutex; quotient_mu last.
class PqCall {
public:
    explicit PqCall(kzg_ctx* ctx, const ProveRound* round = nullptr)
        : ctx_(ctx), lkq_(ctx->quotient_mu, std::defer_lock), own_(ctx->mu, std::defer_lock), lk_(round ? round->lk : &own_),
          lease_{ctx, -1} {
        if (round) {
            slot_ = round->slot;
            drain_.s = &ctx->slots[slot_];
        } else {
            lkq_.lock();
        }
    }
    void lock() {
        if (lk_ == &own_) own_.lock();
    }
    // batch_only: kzg_ntt_batch, which reads the twiddles alone (with the batched kernel's LDS limit) and not the g-power tables
    int begin(bool batch_only = false) {
        if (lk_ != &own_) return KZG_OK;
        HIP_TRY(ctx_, hipSetDevice(ctx_->device));
        int rc = batch_only ? ensure_ntt_batch(ctx_) : ensure_ntt(ctx_);
        if (rc == KZG_OK && !batch_only) rc = ensure_recover_g(ctx_);
        if (rc) return rc;
        slot_ = reserve_slot(ctx_, own_, true);
        if (slot_ < 0) return KZG_ERR_BUSY;
        lease_.slot = slot_;
        drain_.s = &ctx_->slots[slot_];
        return ensure_slot_basics(ctx_, ctx_->slots[slot_]);  // needs no SRS
    }
    std::unique_lock<std::mutex>& lk() const { return *lk_; }
    int slot() const { return slot_; }
    Slot& s() const { return ctx_->slots[slot_]; }
    void drain() const { drain_.now(); }  // before the end, for a caller that frees what the call wrote to
    ~PqCall() {
        static_assert(offsetof(PqCall, lkq_) < offsetof(PqCall, own_) && offsetof(PqCall, own_) < offsetof(PqCall, lease_) &&
                          offsetof(PqCall, lease_) < offsetof(PqCall, drain_),
                      "the order of release");
    }

private:
    kzg_ctx* ctx_;
    int slot_ = -1;
    std::unique_lock<std::mutex> lkq_, own_;  // quotient_mu, ctx->mu
    std::unique_lock<std::mutex>* lk_;        // own_, or the round's
    SlotLease lease_;                         // (no slot: gives nothing back)
    PqDrain drain_;
};

// t columns of len values, column j at src + 4 j stride, packed to stride len at dst
int pq_upload(kzg_ctx* ctx, std::unique_lock<std::mutex>& lk, hipStream_t st, uint32_t* dst, const uint64_t* src, size_t len, size_t t,
              size_t stride) {
    if (stride == len) return copy_unlocked(ctx, lk, st, dst, src, t * len * 32, hipMemcpyHostToDevice, "hipMemcpyAsync (columns)");
    for (size_t j = 0; j < t; j++) {
        int rc = copy_unlocked(ctx, lk, st, dst + 8 * j * len, src + 4 * j * stride, len * 32, hipMemcpyHostToDevice,
                               "hipMemcpyAsync (columns)");
        if (rc) return rc;
    }
    return KZG_OK;
}
// The per-proof columns of a circuit call (t wires at `stride`, z, and PI or null: n values each) where the body reads them.
// Device inputs stay where they are.  Host inputs are packed into d_in, uploaded in the order they lie there: the wires, then
// [ z | PI ] (the quotients: the order of their extended columns) or, z_last, [ PI | z ] (the opening: the order of its stack)
struct PqStaged {
    const uint32_t *w, *z, *pi;
    size_t stride;
};
int pq_stage(kzg_ctx* ctx, std::unique_lock<std::mutex>& lk, hipStream_t st, bool device, uint32_t* d_in, const void* wires,
             size_t stride, const void* z, const void* pi, size_t n, size_t t, bool z_last, PqStaged* out) {
    *out = PqStaged{(const uint32_t*)wires, (const uint32_t*)z, (const uint32_t*)pi, stride};
    if (device) return KZG_OK;
    uint32_t *d_z = d_in + 8 * (t + (z_last && pi ? 1 : 0)) * n, *d_pi = d_in + 8 * (t + (z_last ? 0 : 1)) * n;
    int rc = pq_upload(ctx, lk, st, d_in, (const uint64_t*)wires, n, t, stride);
    if (rc == KZG_OK && pi && z_last) rc = pq_upload(ctx, lk, st, d_pi, (const uint64_t*)pi, n, 1, n);
    if (rc == KZG_OK) rc = pq_upload(ctx, lk, st, d_z, (const uint64_t*)z, n, 1, n);
    if (rc == KZG_OK && pi && !z_last) rc = pq_upload(ctx, lk, st, d_pi, (const uint64_t*)pi, n, 1, n);
    *out = PqStaged{d_in, d_z, pi ? d_pi : nullptr, n};
    return rc;
}

// ---- transforms of a batch of columns (ntt_batch_kernels.hip) -------------------------------------------
// kzg_ntt's argument rules for every column, stride >= n, and extents that fit the address space; *extent: (batch - 1) stride + n
// values, the bytes / 32 a side of the call spans (0 for an empty batch)
bool nttb_args_ok(size_t n, size_t batch, size_t in_stride, size_t out_stride, uint32_t* lg, size_t* in_extent, size_t* out_extent) {
    if (!ntt_log(n, lg) || in_stride < n || out_stride < n) return false;
    const size_t most = ((size_t)1 << 58) / (batch ? batch : 1);  // batch x stride x 32 bytes stays below 2^63
    if (in_stride > most || out_stride > most) return false;
    *in_extent = batch ? (batch - 1) * in_stride + n : 0;
    *out_extent = batch ? (batch - 1) * out_stride + n : 0;
    return true;
}
// in == out with equal strides is the in-place form; any other overlap of the two sides is refused
bool nttb_alias_ok(const void* in, size_t in_extent, size_t in_stride, const void* out, size_t out_extent, size_t out_stride) {
    if (in == out && in_stride == out_stride) return true;
    return !pq_overlap(in, in_extent * 32, out, out_extent * 32);
}
// the twiddles, and the batched pass kernel's LDS limit raised once per context (ctx->mu held, the device current): a refusal
// fails the batched calls alone, with a message of their own
int ensure_ntt_batch(kzg_ctx* ctx) {
    int rc = ensure_ntt(ctx);
    if (rc || ctx->nttb_ready) return rc;
    if (!ntt_batch_prepare_device()) {
        (void)hipGetLastError();
        ctx->last_error = "ntt batch: the batched pass kernel's LDS limit could not be raised";
        return KZG_ERR_HIP;
    }
    ctx->nttb_ready = true;
    return KZG_OK;
}
// columns per round of a batched transform: pq_bufs's share of the budget per buffer, so that KZG_PQ_WS_KB shrinks it
size_t nttb_chunk(const kzg_ctx* ctx, size_t n, size_t batch) {
    size_t chunk = ctx->pq_ws_budget / (4 * n * 32);
    chunk = chunk < 1 ? 1 : (chunk > kPqMaxChunk ? kPqMaxChunk : chunk);
    return chunk > batch ? batch : chunk;
}
// what a batched transform takes from the workspaces: the two intermediates of launch_ntt_batch when the plan has more than one
// pass (a single pass writes none), and for host data the staging buffer; `chunk` columns of n values each
struct NttbBufs {
    uint32_t *stage = nullptr, *a = nullptr, *b = nullptr;
    size_t chunk = 0;
};
// ctx->mu and quotient_mu held
int nttb_bufs(kzg_ctx* ctx, size_t n, uint32_t lg, size_t batch, bool staging, NttbBufs* w) {
    w->chunk = nttb_chunk(ctx, n, batch);
    void* p = nullptr;
    int rc = KZG_OK;
    if (ntt_plan(lg).passes > 1) {
        rc = ctx->pq_ws.get(ctx, kPqA, w->chunk * n * 32, &p);
        w->a = (uint32_t*)p;
        if (rc == KZG_OK) rc = ctx->pq_ws.get(ctx, kPqB, w->chunk * n * 32, &p);
        w->b = (uint32_t*)p;
    }
    if (rc == KZG_OK && staging) {
        rc = ctx->pq_ws.get(ctx, kPqT, w->chunk * n * 32, &p);
        w->stage = (uint32_t*)p;
    }
    return rc;
}
// in, out: host pointers (staged through the workspace, a chunk of columns at a time), or device pointers when `device`
int ntt_batch_impl(kzg_ctx* ctx, const void* in, size_t n, size_t batch, size_t in_stride, void* out, size_t out_stride, bool inverse,
                   bool device) {
    uint32_t lg = 0;
    size_t in_extent = 0, out_extent = 0;
    if (!nttb_args_ok(n, batch, in_stride, out_stride, &lg, &in_extent, &out_extent) ||
        !nttb_alias_ok(in, in_extent, in_stride, out, out_extent, out_stride))
        return KZG_ERR_INVALID_ARG;
    if (!batch) return KZG_OK;
    PqCall call(ctx);
    call.lock();
    int rc = call.begin(true);
    if (rc) return rc;
    std::unique_lock<std::mutex>& lk = call.lk();
    Slot& s = call.s();
    NttbBufs w;
    rc = nttb_bufs(ctx, n, lg, batch, !device, &w);
    if (rc) return rc;
    const Fr30* tw = (const Fr30*)ctx->ntt_tw.p + (inverse ? 2 * kNttTableLen : 0);
    const Fr30 last_c = fr30_arg_from_mont256(inverse ? hf::fr_inv(fr_pow2(lg)) : hf::kFrOne);
    for (size_t c0 = 0; c0 < batch; c0 += w.chunk) {
        const size_t bc = batch - c0 < w.chunk ? batch - c0 : w.chunk;
        if (device) {
            launch_ntt_batch(s.stream, (const uint32_t*)in + 8 * c0 * in_stride, in_stride, (uint32_t*)out + 8 * c0 * out_stride, out_stride,
                             lg, (uint32_t)bc, tw, last_c, w.a, w.b);
            HIP_TRY(ctx, hipGetLastError());
            continue;
        }
        rc = pq_upload(ctx, lk, s.stream, w.stage, (const uint64_t*)in + 4 * c0 * in_stride, n, bc, in_stride);
        if (rc) return rc;
        launch_ntt_batch(s.stream, w.stage, n, w.stage, n, lg, (uint32_t)bc, tw, last_c, w.a, w.b);
        HIP_TRY(ctx, hipGetLastError());
        for (size_t b = 0; b < bc && rc == KZG_OK; b++)
            rc = copy_unlocked(ctx, lk, s.stream, (uint64_t*)out + 4 * (c0 + b) * out_stride, w.stage + 8 * b * n, n * 32,
                               hipMemcpyDeviceToHost, "hipMemcpyAsync (transformed columns)");
        if (rc) return rc;
    }
    return sync_unlocked(ctx, lk, s.stream, "ntt batch");
}
}  // namespace

int kzg_ntt_batch(kzg_ctx* ctx, const uint64_t* in, size_t n, size_t batch, size_t in_stride, int inverse, uint64_t* out,
                  size_t out_stride) {
    if (!ctx || !in || !out) return KZG_ERR_INVALID_ARG;
    if (ctx->multi) {  // needs no SRS
        kzg_ctx* kid = multi_kid(ctx->multi, 0);
        return forwarded(ctx, kid, kzg_ntt_batch(kid, in, n, batch, in_stride, inverse, out, out_stride));
    }
    return ntt_batch_impl(ctx, in, n, batch, in_stride, out, out_stride, inverse != 0, false);
}

int kzg_ntt_batch_rounds(kzg_ctx* ctx, size_t n, size_t batch, size_t* rounds) {
    uint32_t lg = 0;
    if (!ctx || !rounds || !ntt_log(n, &lg)) return KZG_ERR_INVALID_ARG;
    if (ctx->multi) return kzg_ntt_batch_rounds(multi_kid(ctx->multi, 0), n, batch, rounds);
    const size_t chunk = batch ? nttb_chunk(ctx, n, batch) : 1;  // (the budget is fixed when the context is created)
    *rounds = (batch + chunk - 1) / chunk;
    return KZG_OK;
}

int kzg_ntt_batch_device(kzg_ctx* ctx, const void* d_in, size_t n, size_t batch, size_t in_stride, void* d_out, size_t out_stride,
                         int inverse) {
    KZG_SINGLE_DEVICE_ONLY(ctx);
    if (!ctx || !d_in || !d_out) return KZG_ERR_INVALID_ARG;
    return ntt_batch_impl(ctx, d_in, n, batch, in_stride, d_out, out_stride, inverse != 0, true);
}

// `chunks` vectors of n coefficients (vector c at d_coef + 8 c stride words, stride 0: n; resident until the call returns) committed
// over the monomial SRS on the caller's reserved slot: batched MSMs, as many vectors per job as the slot holds
static int pq_commit_chunks(kzg_ctx* ctx, std::unique_lock<std::mutex>& lk, int slot, const uint32_t* d_coef, size_t n, size_t chunks,
                            uint64_t* out_p1s, size_t stride = 0) {
    if (!stride) stride = n;
    if (int rc = pq_srs_status(ctx, true, n)) return rc;  // (the wait for a slot dropped the mutex: the SRS may have changed)
    Slot& s = ctx->slots[slot];
    const size_t group = std::min<size_t>(chunks, ctx->max_batch ? ctx->max_batch : 1);
    for (size_t c0 = 0; c0 < chunks; c0 += group) {
        const size_t g = chunks - c0 < group ? chunks - c0 : group;
        const uint32_t* d_chunk = d_coef + 8 * c0 * stride;
        int rc = g == 1 ? submit_commit_locked(ctx, slot, d_chunk, 1, n, true, true) : commit_batch_submit_locked(ctx, slot, d_chunk, n, g, stride, true);
        if (rc) return rc;
        await_unlocked(lk, s);
        rc = g == 1 ? wait_locked(ctx, slot, out_p1s + 18 * c0) : wait_batch_locked(ctx, slot, out_p1s + 18 * c0, g);
        s.kind = SLOT_RESERVED;  // (the mutex was held since the wait marked it idle)
        if (rc) return rc;
    }
    return KZG_OK;
}

static int coset_extend_impl(kzg_ctx* ctx, const void* in, size_t len, size_t batch, size_t stride, unsigned form, unsigned log_out,
                             void* out, bool device) {
    uint32_t lg_len = 0;
    if (!ctx || !in || !out || log_out > kNttMaxLog || len < 1 || len > ((size_t)1 << log_out) || batch < 1 || stride < len ||
        (form != KZG_EXTEND_VALUES && form != KZG_EXTEND_COEFFS) || (form == KZG_EXTEND_VALUES && !ntt_log(len, &lg_len)))
        return KZG_ERR_INVALID_ARG;
    const size_t N = (size_t)1 << log_out;
    if (device && pq_overlap(out, batch * N * 32, in, ((batch - 1) * stride + len) * 32)) {
        ctx->last_error = "coset extension: the output overlaps the input";
        return KZG_ERR_INVALID_ARG;
    }
    PqCall call(ctx);
    call.lock();
    int rc = call.begin();
    if (rc) return rc;
    std::unique_lock<std::mutex>& lk = call.lk();
    Slot& s = call.s();
    const int lg = form == KZG_EXTEND_VALUES ? (int)lg_len : -1;
    if (device) {
        PqBufs w;
        rc = pq_bufs(ctx, N, batch, &w);
        if (rc == KZG_OK) rc = pq_extend(ctx, s.stream, (const uint32_t*)in, stride, len, lg, batch, log_out, (uint32_t*)out, w);
        return rc ? rc : sync_unlocked(ctx, lk, s.stream, "coset extension");
    }
    // host pointers: as many columns per round as the budget holds, packed on the way up
    size_t round = ctx->pq_ws_budget / (N * 32);
    round = round < 1 ? 1 : (round > batch ? batch : round);
    PqBufs w;
    void *d_in, *d_out;
    rc = pq_bufs(ctx, N, round, &w);
    if (rc == KZG_OK) rc = ctx->pq_ws.get(ctx, kPqIn, round * len * 32, &d_in);
    if (rc == KZG_OK) rc = ctx->pq_ws.get(ctx, kPqCols, round * N * 32, &d_out);
    for (size_t b0 = 0; b0 < batch && rc == KZG_OK; b0 += round) {
        const size_t bc = batch - b0 < round ? batch - b0 : round;
        rc = pq_upload(ctx, lk, s.stream, (uint32_t*)d_in, (const uint64_t*)in + 4 * b0 * stride, len, bc, stride);
        if (rc == KZG_OK) rc = pq_extend(ctx, s.stream, (const uint32_t*)d_in, len, len, lg, bc, log_out, (uint32_t*)d_out, w);
        if (rc == KZG_OK)
            rc = copy_unlocked(ctx, lk, s.stream, (uint64_t*)out + 4 * b0 * N, d_out, bc * N * 32, hipMemcpyDeviceToHost,
                               "hipMemcpyAsync (extended columns)");
        if (rc == KZG_OK) rc = sync_unlocked(ctx, lk, s.stream, "coset extension");
    }
    return rc;
}

int kzg_coset_extend(kzg_ctx* ctx, const uint64_t* in, size_t len, size_t batch, size_t stride, unsigned form, unsigned log_out,
                     uint64_t* out) {
    if (ctx && ctx->multi) {  // needs no SRS
        kzg_ctx* kid = multi_kid(ctx->multi, 0);
        return forwarded(ctx, kid, kzg_coset_extend(kid, in, len, batch, stride, form, log_out, out));
    }
    return coset_extend_impl(ctx, in, len, batch, stride, form, log_out, out, false);
}

int kzg_coset_extend_device(kzg_ctx* ctx, const void* d_in, size_t len, size_t batch, size_t stride, unsigned form, unsigned log_out,
                            void* d_out) {
    KZG_SINGLE_DEVICE_ONLY(ctx);
    return coset_extend_impl(ctx, d_in, len, batch, stride, form, log_out, d_out, true);
}

static bool pq_constraint_args_ok(kzg_ctx* ctx, const void* wires, const void* sigmas, const void* z, size_t n, size_t rot, size_t t,
                                  size_t stride, const uint64_t* shifts, const uint64_t* alpha, const uint64_t* beta,
                                  const uint64_t* gamma, const void* out, PqShape* sh) {
    return ctx && wires && sigmas && z && shifts && alpha && beta && gamma && out && pq_shape(n, rot, sh) && t >= 1 &&
           t <= kPqMaxColumns && t + 1 <= rot && stride >= sh->N;
}

int kzg_permutation_constraints_coset(kzg_ctx* ctx, const uint64_t* wires_ext, const uint64_t* sigmas_ext, const uint64_t* z_ext,
                                      size_t n, size_t rot, size_t t, size_t stride, const uint64_t* shifts, const uint64_t alpha[4],
                                      const uint64_t beta[4], const uint64_t gamma[4], const uint64_t* gate_coset, uint64_t* out) {
    PqShape sh;
    if (!pq_constraint_args_ok(ctx, wires_ext, sigmas_ext, z_ext, n, rot, t, stride, shifts, alpha, beta, gamma, out, &sh))
        return KZG_ERR_INVALID_ARG;
    if (ctx->multi) {  // needs no SRS
        kzg_ctx* kid = multi_kid(ctx->multi, 0);
        return forwarded(ctx, kid, kzg_permutation_constraints_coset(kid, wires_ext, sigmas_ext, z_ext, n, rot, t, stride, shifts, alpha,
                                                                    beta, gamma, gate_coset, out));
    }
    PqCall call(ctx);
    call.lock();
    int rc = call.begin();
    if (rc) return rc;
    std::unique_lock<std::mutex>& lk = call.lk();
    Slot& s = call.s();
    const size_t N = sh.N;
    PqBufs w;
    void *cols, *d_out, *d_gate = nullptr;
    rc = pq_bufs(ctx, N, 1, &w);
    if (rc == KZG_OK) rc = ctx->pq_ws.get(ctx, kPqCols, (2 * t + 2) * N * 32, &cols);  // wires, sigmas, z, L_0
    if (rc == KZG_OK) rc = ctx->pq_ws.get(ctx, kPqOut, N * 32, &d_out);
    if (rc == KZG_OK && gate_coset) rc = ctx->pq_ws.get(ctx, kPqGate, N * 32, &d_gate);
    if (rc) return rc;
    uint32_t *d_w = (uint32_t*)cols, *d_s = d_w + 8 * t * N, *d_z = d_s + 8 * t * N, *d_l0 = d_z + 8 * N;
    rc = pq_upload(ctx, lk, s.stream, d_w, wires_ext, N, t, stride);
    if (rc == KZG_OK) rc = pq_upload(ctx, lk, s.stream, d_s, sigmas_ext, N, t, stride);
    if (rc == KZG_OK) rc = pq_upload(ctx, lk, s.stream, d_z, z_ext, N, 1, N);
    if (rc == KZG_OK && gate_coset) rc = pq_upload(ctx, lk, s.stream, (uint32_t*)d_gate, gate_coset, N, 1, N);
    const PqChallenges ch{shifts, alpha, beta, gamma};
    if (rc == KZG_OK) rc = pq_constraints(ctx, lk, s.stream, sh, t, N, d_w, d_s, d_z, (const uint32_t*)d_gate, d_l0, ch, w, (uint32_t*)d_out);
    if (rc == KZG_OK) rc = copy_unlocked(ctx, lk, s.stream, out, d_out, N * 32, hipMemcpyDeviceToHost, "hipMemcpyAsync (constraints)");
    return rc ? rc : sync_unlocked(ctx, lk, s.stream, "permutation constraints");
}

int kzg_permutation_constraints_coset_device(kzg_ctx* ctx, const void* d_wires_ext, const void* d_sigmas_ext, const void* d_z_ext,
                                             size_t n, size_t rot, size_t t, size_t stride, const uint64_t* shifts,
                                             const uint64_t alpha[4], const uint64_t beta[4], const uint64_t gamma[4],
                                             const void* d_gate_coset, void* d_out) {
    KZG_SINGLE_DEVICE_ONLY(ctx);
    PqShape sh;
    if (!pq_constraint_args_ok(ctx, d_wires_ext, d_sigmas_ext, d_z_ext, n, rot, t, stride, shifts, alpha, beta, gamma, d_out, &sh))
        return KZG_ERR_INVALID_ARG;
    const size_t N = sh.N, span = ((t - 1) * stride + N) * 32;
    if (pq_overlap(d_out, N * 32, d_wires_ext, span) || pq_overlap(d_out, N * 32, d_sigmas_ext, span) ||
        pq_overlap(d_out, N * 32, d_z_ext, N * 32) || (d_gate_coset && pq_overlap(d_out, N * 32, d_gate_coset, N * 32))) {
        ctx->last_error = "permutation constraints: the output overlaps an input";
        return KZG_ERR_INVALID_ARG;
    }
    PqCall call(ctx);
    call.lock();
    int rc = call.begin();
    if (rc) return rc;
    std::unique_lock<std::mutex>& lk = call.lk();
    Slot& s = call.s();
    PqBufs w;
    void* d_l0;
    rc = pq_bufs(ctx, N, 1, &w);
    if (rc == KZG_OK) rc = ctx->pq_ws.get(ctx, kPqCols, N * 32, &d_l0);
    const PqChallenges ch{shifts, alpha, beta, gamma};
    if (rc == KZG_OK)
        rc = pq_constraints(ctx, lk, s.stream, sh, t, stride, (const uint32_t*)d_wires_ext, (const uint32_t*)d_sigmas_ext,
                            (const uint32_t*)d_z_ext, (const uint32_t*)d_gate_coset, (uint32_t*)d_l0, ch, w, (uint32_t*)d_out);
    return rc ? rc : sync_unlocked(ctx, lk, s.stream, "permutation constraints");
}

static int vanishing_quotient_impl(kzg_ctx* ctx, const void* num, size_t N, size_t n, int already_divided, void* out, bool device) {
    PqShape sh;
    if (!ctx || !num || !out || n < 1 || N < n || N % n || !pq_shape(n, N / n, &sh)) return KZG_ERR_INVALID_ARG;
    if (device && pq_overlap(out, (N - n) * 32, num, N * 32)) {
        ctx->last_error = "vanishing quotient: the output overlaps the input";
        return KZG_ERR_INVALID_ARG;
    }
    PqCall call(ctx);
    call.lock();
    int rc = call.begin();
    if (rc) return rc;
    std::unique_lock<std::mutex>& lk = call.lk();
    Slot& s = call.s();
    PqBufs w;
    void *vals, *coef = out, *flag;
    rc = pq_bufs(ctx, N, 1, &w);
    if (rc == KZG_OK) rc = ctx->pq_ws.get(ctx, kPqOut, N * 32, &vals);
    if (rc == KZG_OK && !device) rc = ctx->pq_ws.get(ctx, kPqCoef, (N - n) * 32, &coef);
    if (rc == KZG_OK) rc = ctx->pq_ws.get(ctx, kPqFlag, 4, &flag);
    if (rc) return rc;
    // the values go into the workspace, where the division may change them
    rc = copy_unlocked(ctx, lk, s.stream, vals, num, N * 32, device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice,
                       "hipMemcpyAsync (numerator)");
    bool remainder = false;
    if (rc == KZG_OK)
        rc = pq_finish(ctx, lk, s.stream, sh, (uint32_t*)vals, !already_divided, w, (uint32_t*)coef, (uint32_t*)flag, 0, N - n,
                       device ? nullptr : out, "vanishing quotient", &remainder);
    if (rc) return rc;
    return remainder ? pq_remainder(ctx, sh) : KZG_OK;
}

int kzg_vanishing_quotient(kzg_ctx* ctx, const uint64_t* num_coset, size_t N, size_t n, int already_divided, uint64_t* out_coeffs) {
    if (ctx && ctx->multi) {  // needs no SRS
        kzg_ctx* kid = multi_kid(ctx->multi, 0);
        return forwarded(ctx, kid, kzg_vanishing_quotient(kid, num_coset, N, n, already_divided, out_coeffs));
    }
    return vanishing_quotient_impl(ctx, num_coset, N, n, already_divided, out_coeffs, false);
}

int kzg_vanishing_quotient_device(kzg_ctx* ctx, const void* d_num_coset, size_t N, size_t n, int already_divided, void* d_out_coeffs) {
    KZG_SINGLE_DEVICE_ONLY(ctx);
    return vanishing_quotient_impl(ctx, d_num_coset, N, n, already_divided, d_out_coeffs, true);
}

int kzg_permutation_quotient(kzg_ctx* ctx, const uint64_t* wires, const uint64_t* sigmas, const uint64_t* z, size_t n, size_t t,
                             size_t stride, const uint64_t* shifts, const uint64_t alpha[4], const uint64_t beta[4],
                             const uint64_t gamma[4], const uint64_t* gate_coset, unsigned log_ext, uint64_t* out_coeffs,
                             uint64_t* out_p1s) {
    PqShape sh;
    if (!ctx || log_ext > kPqMaxLogExt || !pq_shape(n, (size_t)1 << log_ext, &sh) || t < 1 || t + 1 > sh.rot || stride < n || !wires ||
        !sigmas || !z || !shifts || !alpha || !beta || !gamma)
        return KZG_ERR_INVALID_ARG;
    if (ctx->multi) {
        kzg_ctx* kid = whole_srs_kid(ctx, out_p1s != nullptr, "the quotient's commitments need");
        if (!kid) return KZG_ERR_INVALID_ARG;
        return forwarded(ctx, kid, kzg_permutation_quotient(kid, wires, sigmas, z, n, t, stride, shifts, alpha, beta, gamma, gate_coset,
                                                           log_ext, out_coeffs, out_p1s));
    }
    PqCall call(ctx);
    call.lock();
    int rc = pq_srs_status(ctx, out_p1s != nullptr, n);
    if (rc == KZG_OK) rc = call.begin();
    if (rc) return rc;
    std::unique_lock<std::mutex>& lk = call.lk();
    Slot& s = call.s();
    const size_t N = sh.N, ncols = 2 * t + 1;
    PqBufs w;
    void *in, *cols, *d_out, *coef, *flag, *d_gate = nullptr;
    rc = pq_bufs(ctx, N, ncols, &w);
    if (rc == KZG_OK) rc = ctx->pq_ws.get(ctx, kPqIn, ncols * n * 32, &in);
    if (rc == KZG_OK) rc = ctx->pq_ws.get(ctx, kPqCols, (ncols + 1) * N * 32, &cols);  // wires, sigmas, z, L_0
    if (rc == KZG_OK) rc = ctx->pq_ws.get(ctx, kPqOut, N * 32, &d_out);
    if (rc == KZG_OK) rc = ctx->pq_ws.get(ctx, kPqCoef, (N - n) * 32, &coef);
    if (rc == KZG_OK) rc = ctx->pq_ws.get(ctx, kPqFlag, 4, &flag);
    if (rc == KZG_OK && gate_coset) rc = ctx->pq_ws.get(ctx, kPqGate, N * 32, &d_gate);
    if (rc) return rc;
    uint32_t* d_in = (uint32_t*)in;
    uint32_t *d_w = (uint32_t*)cols, *d_s = d_w + 8 * t * N, *d_z = d_s + 8 * t * N, *d_l0 = d_z + 8 * N;
    rc = pq_upload(ctx, lk, s.stream, d_in, wires, n, t, stride);
    if (rc == KZG_OK) rc = pq_upload(ctx, lk, s.stream, d_in + 8 * t * n, sigmas, n, t, stride);
    if (rc == KZG_OK) rc = pq_upload(ctx, lk, s.stream, d_in + 16 * t * n, z, n, 1, n);
    if (rc == KZG_OK && gate_coset) rc = pq_upload(ctx, lk, s.stream, (uint32_t*)d_gate, gate_coset, N, 1, N);
    if (rc == KZG_OK) rc = pq_extend(ctx, s.stream, d_in, n, n, (int)sh.lg_n, ncols, sh.lg_N, d_w, w);
    const PqChallenges ch{shifts, alpha, beta, gamma};
    if (rc == KZG_OK) rc = pq_constraints(ctx, lk, s.stream, sh, t, N, d_w, d_s, d_z, (const uint32_t*)d_gate, d_l0, ch, w, (uint32_t*)d_out);
    bool remainder = false;
    if (rc == KZG_OK)
        rc = pq_finish(ctx, lk, s.stream, sh, (uint32_t*)d_out, false, w, (uint32_t*)coef, (uint32_t*)flag, 0, N - n, out_coeffs,
                       "permutation quotient", &remainder);
    if (rc) return rc;
    if (remainder) return pq_remainder(ctx, sh);
    if (!out_p1s) return KZG_OK;
    return pq_commit_chunks(ctx, lk, call.slot(), (const uint32_t*)coef, n, sh.rot - 1, out_p1s);
}

// ---- a circuit's key resident on the device (circuit_kernels.hip) -----------------------------------------
// The calls hold quotient_mu, then the context's mutex and one slot, as the quotient's calls above; the per-proof columns live in
// pq_ws, the circuit's buffers are written by kzg_circuit_create alone.
static size_t circuit_column_index(const kzg_circuit* c, unsigned which) {
    if (which >= KZG_CIRCUIT_COL_QLIN && which < KZG_CIRCUIT_COL_QLIN + c->t) return which - KZG_CIRCUIT_COL_QLIN;
    if (which == KZG_CIRCUIT_COL_QM) return c->t;
    if (which == KZG_CIRCUIT_COL_QC) return c->t + 1;
    if (which >= KZG_CIRCUIT_COL_SIGMA && which < KZG_CIRCUIT_COL_SIGMA + c->t) return c->t + 2 + (which - KZG_CIRCUIT_COL_SIGMA);
    if (which >= KZG_CIRCUIT_COL_TABLE && which < KZG_CIRCUIT_COL_TABLE + c->c_tab) return 2 * c->t + 2 + (which - KZG_CIRCUIT_COL_TABLE);
    if (which == KZG_CIRCUIT_COL_QLOOKUP && c->c_tab) return 2 * c->t + 2 + c->c_tab;
    if (which >= KZG_CIRCUIT_COL_CUSTOM && which < KZG_CIRCUIT_COL_CUSTOM + c->g_custom) return 2 * c->t + 2 + (which - KZG_CIRCUIT_COL_CUSTOM);
    return (size_t)-1;
}
// is `c` a circuit alive on the single-device context `ctx` (quotient_mu held)?
static bool circuit_alive(kzg_ctx* ctx, const kzg_circuit* c) {
    return c && std::find(ctx->circuits.begin(), ctx->circuits.end(), c) != ctx->circuits.end();
}
static int circuit_foreign(kzg_ctx* ctx) {
    ctx->last_error = "circuit: the handle is not a circuit alive on this context";
    return KZG_ERR_INVALID_ARG;
}

// the body of kzg_circuit_create on a single-device context (on its frame: quotient_mu held): fills *c, whose buffers go with it
// on failure.  The frame is the caller's, because quotient_mu has to outlast this body (the list of circuits): the context's
// mutex and the slot are therefore held until kzg_circuit_create returns -- on failure across the drain and the hipFree of c's
// buffers, which take no lock
struct CircuitTable {  // the columns of a lookup circuit (section 4.26): c table columns at a stride and q_K, or c = 0
    const uint64_t* table = nullptr;
    size_t c = 0, stride = 0;
    const uint64_t* q_lookup = nullptr;
    // ... or of a custom circuit (section 4.27): g selector columns at a stride, or g = 0 (the exponents are in *c already)
    const uint64_t* q_custom = nullptr;
    size_t g = 0, custom_stride = 0;
};
static int circuit_build(kzg_ctx* ctx, PqCall& call, kzg_circuit* c, const PqShape& sh, const uint64_t* q_lin, const uint64_t* q_mul,
                         const uint64_t* q_const, const uint64_t* sigmas, size_t stride, const CircuitTable& tab,
                         uint64_t* out_key_p1s) {
    call.lock();
    const size_t n = sh.n, N = sh.N, t = c->t, ncols = c->cols();
    int rc = pq_srs_status(ctx, out_key_p1s != nullptr, n);
    if (rc == KZG_OK) rc = call.begin();
    if (rc) return rc;
    std::unique_lock<std::mutex>& lk = call.lk();
    Slot& s = call.s();
    PqBufs w;
    rc = pq_bufs(ctx, N, ncols, &w);
    if (rc == KZG_OK) rc = c->values.reserve(ctx, ncols * n * 32);
    if (rc == KZG_OK) rc = c->coeffs.reserve(ctx, ncols * n * 32);
    if (rc == KZG_OK) rc = c->coset.reserve(ctx, ncols * N * 32);
    if (rc == KZG_OK) rc = c->l0.reserve(ctx, N * 32);
    if (rc == KZG_OK) rc = c->zinv.reserve(ctx, 8 * 32);
    if (rc) return rc;
    uint32_t *d_val = c->values.dev(), *d_coef = c->coeffs.dev();
    rc = pq_upload(ctx, lk, s.stream, d_val, q_lin, n, t, stride);
    if (rc == KZG_OK) rc = pq_upload(ctx, lk, s.stream, d_val + 8 * t * n, q_mul, n, 1, n);
    if (rc == KZG_OK) rc = pq_upload(ctx, lk, s.stream, d_val + 8 * (t + 1) * n, q_const, n, 1, n);
    if (rc == KZG_OK) rc = pq_upload(ctx, lk, s.stream, d_val + 8 * (t + 2) * n, sigmas, n, t, stride);
    if (rc == KZG_OK && tab.c) rc = pq_upload(ctx, lk, s.stream, d_val + 8 * (2 * t + 2) * n, tab.table, n, tab.c, tab.stride);
    if (rc == KZG_OK && tab.c) rc = pq_upload(ctx, lk, s.stream, d_val + 8 * (2 * t + 2 + tab.c) * n, tab.q_lookup, n, 1, n);
    if (rc == KZG_OK && tab.g) rc = pq_upload(ctx, lk, s.stream, d_val + 8 * (2 * t + 2) * n, tab.q_custom, n, tab.g, tab.custom_stride);
    if (rc) return rc;
    // values -> coefficients (the inverse transform the extension needs anyway, kept) -> the coset
    const Fr30* itw = (const Fr30*)ctx->ntt_tw.p + 2 * kNttTableLen;
    const hf::Fr inv_n_fr = hf::fr_inv(fr_pow2(sh.lg_n));
    const Fr30 inv_n_mul = fr30_arg_from_mont256(inv_n_fr);
    for (size_t b = 0; b < ncols; b++) launch_ntt(s.stream, d_val + 8 * b * n, d_coef + 8 * b * n, sh.lg_n, itw, inv_n_mul, w.A, w.B);
    HIP_TRY(ctx, hipGetLastError());
    rc = pq_extend(ctx, s.stream, d_coef, n, n, -1, ncols, sh.lg_N, c->coset.dev(), w);
    // L_0 = (1 / n) (1 + X + .. + X^(n-1)): from n equal coefficients
    const Fr30 inv_n = pq_image(inv_n_fr);
    if (rc == KZG_OK) rc = pq_extend(ctx, s.stream, nullptr, 0, n, -1, 1, sh.lg_N, c->l0.dev(), w, &inv_n);
    if (rc) return rc;
    // the rot stored multipliers 1 / Z_H(x_i), Z_H(x_i) = g^n w_rot^(i mod rot) - 1 (as pq_upload_zinv makes them)
    uint64_t h[8][4];
    const hf::Fr we = hf::fr_domain_root(sh.lg_ext), k14 = fr_pow2(14);
    hf::Fr cur = hf::fr_pow(fr_seven(), sh.n);
    for (size_t k = 0; k < sh.rot; k++) {
        const hf::Fr stored = hf::fr_mul(hf::fr_inv(hf::fr_sub(cur, hf::kFrOne)), k14);
        std::memcpy(h[k], stored.l, 32);
        cur = hf::fr_mul(cur, we);
    }
    rc = copy_unlocked(ctx, lk, s.stream, c->zinv.p, h, sh.rot * 32, hipMemcpyHostToDevice, "hipMemcpyAsync (vanishing inverses)");
    if (rc == KZG_OK) rc = sync_unlocked(ctx, lk, s.stream, "circuit key");  // (h leaves scope)
    if (rc || !out_key_p1s) return rc;
    return pq_commit_chunks(ctx, lk, call.slot(), d_coef, n, ncols, out_key_p1s);
}

// the shape rules of a lookup circuit (section 4.26): 1 <= c <= t, deg G' = 4 (n - 1) asks for e >= 4, and the last round's
// combination at zeta has 3 t + e + c + 5 columns
static bool lookup_shape_ok(size_t t, size_t e, size_t c) {
    return c >= 1 && c <= t && e >= 4 && e >= t + 1 && 3 * t + e + c + 5 <= kLinMaxColumns;
}
// the shape rules of a custom circuit (section 4.27): 1 <= g <= 8 terms, every exponent in 0..7 and every term of degree d_s >= 1
// (degree 0 is q_C), deg G' <= (d_max + 1) (n - 1) asks for e >= d_max + 1, and the last round's combination at zeta has the plain
// proof's 3 t + e + 3 columns and g more.  *d_max: the largest d_s
// exps_next (or null): the second matrix of a next-row circuit (section 4.28), whose exponents count towards d_s
static bool custom_shape_ok(size_t t, size_t e, size_t g, const uint8_t* exps, size_t* d_max, const uint8_t* exps_next = nullptr) {
    if (!exps || g < 1 || g > kCgMaxTerms || t < 1 || t > kPqMaxColumns || e < t + 1 || 3 * t + e + 3 + g > kLinMaxColumns) return false;
    size_t dm = 0;
    for (size_t s = 0; s < g; s++) {
        size_t d = 0;
        for (size_t j = 0; j < t; j++) {
            if (exps[s * t + j] > 7 || (exps_next && exps_next[s * t + j] > 7)) return false;
            d += exps[s * t + j] + (exps_next ? exps_next[s * t + j] : 0);
        }
        if (d < 1) return false;
        dm = d > dm ? d : dm;
    }
    if (d_max) *d_max = dm;
    return e >= dm + 1;
}
// the shape rules of a next-row circuit (section 4.28): custom_shape_ok's with d_s over both matrices, n >= 2 (at n = 1 the sets
// {zeta, zeta w} would hold one point twice) and rho >= 1 wires with a next-row exponent (none: that is a custom circuit).
// next_wires (or null): those wires, ascending; returns rho, 0 for a shape that is refused
static size_t next_shape_rho(size_t n, size_t t, size_t e, size_t g, const uint8_t* exps, const uint8_t* exps_next, size_t* d_max,
                             uint8_t* next_wires) {
    if (n < 2 || !exps_next || !custom_shape_ok(t, e, g, exps, d_max, exps_next)) return 0;
    size_t rho = 0;
    for (size_t j = 0; j < t; j++) {
        bool used = false;
        for (size_t s = 0; s < g; s++) used = used || exps_next[s * t + j] != 0;
        if (!used) continue;
        if (next_wires) next_wires[rho] = (uint8_t)j;
        rho++;
    }
    return rho;
}
// kzg_circuit_create, kzg_circuit_create_lookup (tab.c != 0), kzg_circuit_create_custom (tab.g != 0, exps: its g t exponents) and
// kzg_circuit_create_custom_next (exps_next too) after their argument checks, on a single-device context
static int circuit_create_impl(kzg_ctx* ctx, const PqShape& sh, const uint64_t* q_lin, const uint64_t* q_mul, const uint64_t* q_const,
                               const uint64_t* sigmas, size_t t, size_t stride, const uint64_t* shifts, const CircuitTable& tab,
                               uint64_t* out_key_p1s, kzg_circuit** out, const uint8_t* exps = nullptr,
                               const uint8_t* exps_next = nullptr) {
    const size_t n = sh.n;
    PqCall call(ctx);
    kzg_circuit* c = new kzg_circuit();
    c->owner = ctx;
    c->lg_n = sh.lg_n;
    c->lg_ext = sh.lg_ext;
    c->n = n;
    c->t = t;
    c->c_tab = tab.c;
    if (tab.g) {
        c->g_custom = tab.g;
        std::memcpy(c->exps, exps, tab.g * t);
        (void)custom_shape_ok(t, sh.rot, tab.g, exps, &c->d_max);
        if (exps_next) {
            std::memcpy(c->exps_next, exps_next, tab.g * t);
            c->rho = next_shape_rho(n, t, sh.rot, tab.g, exps, exps_next, &c->d_max, c->next_wires);
        }
    }
    std::memcpy(c->shifts, shifts, 32 * t);
    int rc = circuit_build(ctx, call, c, sh, q_lin, q_mul, q_const, sigmas, stride, tab, out_key_p1s);
    if (rc) {
        (void)hipSetDevice(ctx->device);
        call.drain();  // (nothing enqueued still writes to the buffers that go with c)
        delete c;
        return rc;
    }
    ctx->circuits.push_back(c);
    *out = c;
    return KZG_OK;
}

int kzg_circuit_create(kzg_ctx* ctx, const uint64_t* q_lin, const uint64_t* q_mul, const uint64_t* q_const, const uint64_t* sigmas,
                       size_t n, size_t t, size_t stride, const uint64_t* shifts, unsigned log_ext, uint64_t* out_key_p1s,
                       kzg_circuit** out) {
    if (out) *out = nullptr;
    PqShape sh;
    if (!ctx || !out || log_ext > kPqMaxLogExt || !pq_shape(n, (size_t)1 << log_ext, &sh) || t < KZG_CIRCUIT_MIN_COLUMNS ||
        t > kPqMaxColumns || t + 1 > sh.rot || stride < n || !q_lin || !q_mul || !q_const || !sigmas || !shifts)
        return KZG_ERR_INVALID_ARG;
    if (ctx->multi) {
        kzg_ctx* kid = whole_srs_kid(ctx, out_key_p1s != nullptr, "the key's commitments need");
        if (!kid) return KZG_ERR_INVALID_ARG;
        return forwarded(ctx, kid, kzg_circuit_create(kid, q_lin, q_mul, q_const, sigmas, n, t, stride, shifts, log_ext, out_key_p1s, out));
    }
    return circuit_create_impl(ctx, sh, q_lin, q_mul, q_const, sigmas, t, stride, shifts, CircuitTable{}, out_key_p1s, out);
}

int kzg_circuit_create_lookup(kzg_ctx* ctx, const uint64_t* q_lin, const uint64_t* q_mul, const uint64_t* q_const, const uint64_t* sigmas,
                              size_t n, size_t t, size_t stride, const uint64_t* shifts, unsigned log_ext, const uint64_t* table, size_t c,
                              size_t table_stride, const uint64_t* q_lookup, uint64_t* out_key_p1s, kzg_circuit** out) {
    if (out) *out = nullptr;
    PqShape sh;
    if (!ctx || !out || log_ext > kPqMaxLogExt || !pq_shape(n, (size_t)1 << log_ext, &sh) || t < KZG_CIRCUIT_MIN_COLUMNS ||
        t > kPqMaxColumns || !lookup_shape_ok(t, sh.rot, c) || stride < n || table_stride < n || !q_lin || !q_mul || !q_const ||
        !sigmas || !shifts || !table || !q_lookup)
        return KZG_ERR_INVALID_ARG;
    if (ctx->multi) {
        kzg_ctx* kid = whole_srs_kid(ctx, out_key_p1s != nullptr, "the key's commitments need");
        if (!kid) return KZG_ERR_INVALID_ARG;
        return forwarded(ctx, kid, kzg_circuit_create_lookup(kid, q_lin, q_mul, q_const, sigmas, n, t, stride, shifts, log_ext, table, c,
                                                            table_stride, q_lookup, out_key_p1s, out));
    }
    return circuit_create_impl(ctx, sh, q_lin, q_mul, q_const, sigmas, t, stride, shifts, CircuitTable{table, c, table_stride, q_lookup},
                               out_key_p1s, out);
}

// kzg_circuit_create_custom (exponents_next null) and kzg_circuit_create_custom_next
static int circuit_create_custom(kzg_ctx* ctx, const uint64_t* q_lin, const uint64_t* q_mul, const uint64_t* q_const, const uint64_t* sigmas,
                                 size_t n, size_t t, size_t stride, const uint64_t* shifts, unsigned log_ext, const uint64_t* q_custom, size_t g,
                                 size_t custom_stride, const uint8_t* exponents, const uint8_t* exponents_next, bool next,
                                 uint64_t* out_key_p1s, kzg_circuit** out) {
    if (out) *out = nullptr;
    PqShape sh;
    if (!ctx || !out || log_ext > kPqMaxLogExt || !pq_shape(n, (size_t)1 << log_ext, &sh) || t < KZG_CIRCUIT_MIN_COLUMNS ||
        t > kPqMaxColumns || stride < n || custom_stride < n || !q_lin || !q_mul || !q_const || !sigmas || !shifts || !q_custom)
        return KZG_ERR_INVALID_ARG;
    if (next ? !next_shape_rho(n, t, sh.rot, g, exponents, exponents_next, nullptr, nullptr)
             : !custom_shape_ok(t, sh.rot, g, exponents, nullptr))
        return KZG_ERR_INVALID_ARG;
    if (ctx->multi) {
        kzg_ctx* kid = whole_srs_kid(ctx, out_key_p1s != nullptr, "the key's commitments need");
        if (!kid) return KZG_ERR_INVALID_ARG;
        return forwarded(ctx, kid, circuit_create_custom(kid, q_lin, q_mul, q_const, sigmas, n, t, stride, shifts, log_ext, q_custom, g,
                                                        custom_stride, exponents, exponents_next, next, out_key_p1s, out));
    }
    CircuitTable tab;
    tab.q_custom = q_custom;
    tab.g = g;
    tab.custom_stride = custom_stride;
    return circuit_create_impl(ctx, sh, q_lin, q_mul, q_const, sigmas, t, stride, shifts, tab, out_key_p1s, out, exponents,
                               next ? exponents_next : nullptr);
}

int kzg_circuit_create_custom(kzg_ctx* ctx, const uint64_t* q_lin, const uint64_t* q_mul, const uint64_t* q_const, const uint64_t* sigmas,
                              size_t n, size_t t, size_t stride, const uint64_t* shifts, unsigned log_ext, const uint64_t* q_custom, size_t g,
                              size_t custom_stride, const uint8_t* exponents, uint64_t* out_key_p1s, kzg_circuit** out) {
    return circuit_create_custom(ctx, q_lin, q_mul, q_const, sigmas, n, t, stride, shifts, log_ext, q_custom, g, custom_stride, exponents,
                                 nullptr, false, out_key_p1s, out);
}

int kzg_circuit_create_custom_next(kzg_ctx* ctx, const uint64_t* q_lin, const uint64_t* q_mul, const uint64_t* q_const,
                                   const uint64_t* sigmas, size_t n, size_t t, size_t stride, const uint64_t* shifts, unsigned log_ext,
                                   const uint64_t* q_custom, size_t g, size_t custom_stride, const uint8_t* exponents,
                                   const uint8_t* exponents_next, uint64_t* out_key_p1s, kzg_circuit** out) {
    return circuit_create_custom(ctx, q_lin, q_mul, q_const, sigmas, n, t, stride, shifts, log_ext, q_custom, g, custom_stride, exponents,
                                 exponents_next, true, out_key_p1s, out);
}

int kzg_circuit_destroy(kzg_ctx* ctx, kzg_circuit* circuit) {
    if (!ctx || !circuit) return KZG_ERR_INVALID_ARG;
    if (ctx->multi) {
        kzg_ctx* kid = multi_kid(ctx->multi, 0);
        return forwarded(ctx, kid, kzg_circuit_destroy(kid, circuit));
    }
    std::lock_guard<std::mutex> lkq(ctx->quotient_mu);  // no quotient runs on it now
    if (!circuit_alive(ctx, circuit)) return circuit_foreign(ctx);
    std::unique_lock<std::mutex> lk(ctx->mu);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    // a caller may still have work of its own queued on the columns it was handed (an opening over the coefficients)
    for (hipStream_t st : {ctx->front_stream, ctx->heavy_stream, ctx->tail_stream})
        if (st) HIP_TRY(ctx, hipStreamSynchronize(st));
    ctx->circuits.erase(std::find(ctx->circuits.begin(), ctx->circuits.end(), circuit));
    delete circuit;
    return KZG_OK;
}

int kzg_circuit_column_device(kzg_ctx* ctx, const kzg_circuit* circuit, unsigned which, unsigned form, const void** d_ptr, size_t* len) {
    if (!ctx || !circuit || !d_ptr || !len) return KZG_ERR_INVALID_ARG;
    if (ctx->multi) {
        kzg_ctx* kid = multi_kid(ctx->multi, 0);
        return forwarded(ctx, kid, kzg_circuit_column_device(kid, circuit, which, form, d_ptr, len));
    }
    std::lock_guard<std::mutex> lkq(ctx->quotient_mu);
    if (!circuit_alive(ctx, circuit)) return circuit_foreign(ctx);
    const size_t n = circuit->n, N = circuit->N();
    if (which == KZG_CIRCUIT_COL_L0) {
        if (form != KZG_CIRCUIT_COSET) return KZG_ERR_INVALID_ARG;
        *d_ptr = circuit->l0.p;
        *len = N;
        return KZG_OK;
    }
    const size_t col = circuit_column_index(circuit, which);
    if (col == (size_t)-1 || form > KZG_CIRCUIT_COSET) return KZG_ERR_INVALID_ARG;
    const DevBuf& b = form == KZG_CIRCUIT_VALUES ? circuit->values : (form == KZG_CIRCUIT_COEFFS ? circuit->coeffs : circuit->coset);
    *len = form == KZG_CIRCUIT_COSET ? N : n;
    *d_ptr = b.dev() + 8 * col * *len;
    return KZG_OK;
}

// The lookup's scalars as its kernels take them (engine.h, LkScalars), for c table columns: theta^j, 2^14, alpha 2^14 and alpha^3
// in multiplier form; beta as the digits of its image.  The kernels' bound comments rest on these magnitudes (canonical residues):
// they are made here and nowhere else.
struct LkKernelScalars {
    Fr30 theta[kPqMaxColumns], beta, k14, ak14, a3;
    LkKernelScalars(const uint64_t* th, const uint64_t* b, const uint64_t* alpha, size_t c) {
        const hf::Fr x = pq_fr(th);
        hf::Fr p = hf::kFrOne;
        for (size_t j = 0; j < c && j < kPqMaxColumns; j++) {
            theta[j] = fr30_arg_from_mont256(p);
            p = hf::fr_mul(p, x);
        }
        beta = pq_image(b ? pq_fr(b) : hf::kFrOne);
        k14 = fr30_arg_from_mont256(fr_pow2(14));
        const hf::Fr a = alpha ? pq_fr(alpha) : hf::kFrOne;
        ak14 = fr30_arg_from_mont256(hf::fr_mul(a, fr_pow2(14)));
        a3 = fr30_arg_from_mont256(hf::fr_mul(hf::fr_mul(a, a), a));
    }
    LkScalars view() const { return LkScalars{theta, &beta, &k14, &ak14, &a3}; }
};
// the lookup of a quotient or of an opening (section 4.26): the multiplicities and the running sum (n values each, where the wires
// are: host or device) and theta; the call's beta is the lookup's.  In a round of kzg_circuit_lookup_prove the two pointers only say
// what is there: the resident coefficients go on behind z with phi, then m: [ f_0 .. f_(t-1) | PI | z | phi | m ].
struct LookupRecord {
    const void *mult, *phi;
    const uint64_t* theta;
};
// the custom gates of a quotient or of an opening (section 4.27): the selectors and the exponents are the circuit's own, so the
// record only says that the call wants the terms: with it the quotient's numerator gains G' = sum_s qx_s prod_j f_j^p[s][j] and
// the last round's r gains sum_s (prod_j abar_j^p[s][j]) qx_s(X)
// A next-row circuit's record (section 4.28) also carries rho >= 1: G' reads the wires at the next row (k_cgn_gate), the last round
// opens the rho wires of next_wires at zeta w too and r gains sum_s (prod_j abar_j^p[s][j] abar'_j^p'[s][j]) qx_s(X)
struct CustomRecord {
    size_t g, d_max;
    const uint8_t* exps;
    size_t rho = 0;
    const uint8_t* exps_next = nullptr;
    const uint8_t* next_wires = nullptr;
};
static int custom_refused(kzg_ctx* ctx, const char* what) {
    ctx->last_error = std::string(what) + ": the circuit was created without custom gates";
    return KZG_ERR_INVALID_ARG;
}
// a call of section 4.27 on a next-row handle would ignore p' and prove a different statement; a call of section 4.28 needs p'
static int custom_kind_refused(kzg_ctx* ctx, const char* what, bool want_next) {
    ctx->last_error = std::string(what) + (want_next ? ": the circuit was created without next-row terms (kzg_circuit_create_custom_next)"
                                                     : ": the circuit has next-row terms, which the kzg_circuit_custom_next_* calls take");
    return KZG_ERR_INVALID_ARG;
}
// G' of the circuit's custom gates from the t extended wire columns at d_w (column j at + 8 j N words) into d_gate (N values):
// k_cgn_gate for a next-row circuit (the next row is e = N / n points on), k_cg_gate otherwise
static int cg_enqueue(kzg_ctx* ctx, hipStream_t stream, const kzg_circuit* c, const PqShape& sh, const uint32_t* d_w, uint32_t* d_gate) {
    const uint32_t* qx = c->coset.dev() + 8 * (2 * c->t + 2) * sh.N;
    if (c->rho)
        launch_cgn_gate(stream, d_w, sh.N, qx, (uint32_t)sh.N, (uint32_t)sh.rot, (uint32_t)c->t, (uint32_t)c->g_custom, c->exps, c->exps_next,
                        fr30_arg_from_mont256(fr_pow2(14)), d_gate);
    else
        launch_cg_gate(stream, d_w, sh.N, qx, (uint32_t)sh.N, (uint32_t)c->t, (uint32_t)c->g_custom, c->exps, fr30_arg_from_mont256(fr_pow2(14)),
                       d_gate);
    HIP_TRY(ctx, hipGetLastError());
    return KZG_OK;
}

// wires (t columns of n values), z, pi (n values or null) and gate (N values or null) are host pointers, or device pointers
// when `device`; then out_coeffs is a device pointer and out_p1s null.  With a lookup record (and no gate) m and phi are extended
// with the wires and k_lk_constraints fills the gate's workspace with G' before the constraint kernel reads it; with a custom record
// (and neither a gate nor a lookup) k_cg_gate fills it from the extended wires.
static int circuit_quotient_impl(kzg_ctx* ctx, const kzg_circuit* c, const void* wires, size_t stride, const void* z, const void* pi,
                                 const uint64_t* alpha, const uint64_t* beta, const uint64_t* gamma, const void* gate, void* out_coeffs,
                                 uint64_t* out_p1s, bool device, const ProveRound* round = nullptr, const LookupRecord* lookup = nullptr,
                                 const CustomRecord* custom = nullptr) {
    PqCall call(ctx, round);
    if (!circuit_alive(ctx, c)) return circuit_foreign(ctx);
    PqShape sh;
    if (!pq_shape(c->n, (size_t)1 << c->lg_ext, &sh) || stride < c->n) return KZG_ERR_INVALID_ARG;
    if (lookup && (!c->c_tab || gate)) {
        ctx->last_error = "circuit lookup quotient: the circuit was created without a lookup table";
        return KZG_ERR_INVALID_ARG;
    }
    if (custom && (!c->g_custom || gate || lookup)) return custom_refused(ctx, "circuit custom quotient");
    if (custom && custom->rho != c->rho) return custom_kind_refused(ctx, "circuit custom quotient", custom->rho != 0);
    const size_t n = sh.n, N = sh.N, t = c->t, nbase = t + 1 + (pi ? 1 : 0), ncols = nbase + (lookup ? 2 : 0);
    if (device) {
        const size_t ob = (N - n) * 32;
        if (pq_overlap(out_coeffs, ob, wires, ((t - 1) * stride + n) * 32) || pq_overlap(out_coeffs, ob, z, n * 32) ||
            (pi && pq_overlap(out_coeffs, ob, pi, n * 32)) || (gate && pq_overlap(out_coeffs, ob, gate, N * 32))) {
            ctx->last_error = "circuit quotient: the output overlaps an input";
            return KZG_ERR_INVALID_ARG;
        }
    }
    call.lock();
    int rc = pq_srs_status(ctx, out_p1s != nullptr, n);
    if (rc == KZG_OK) rc = call.begin();
    if (rc) return rc;
    std::unique_lock<std::mutex>& lk = call.lk();
    Slot& s = call.s();
    PqBufs w;
    void *in = nullptr, *cols, *d_out, *coef = out_coeffs, *flag, *d_gate = const_cast<void*>(gate);
    rc = pq_bufs(ctx, N, ncols, &w);
    if (rc == KZG_OK && !device) rc = ctx->pq_ws.get(ctx, kPqIn, ncols * n * 32, &in);
    if (rc == KZG_OK) rc = ctx->pq_ws.get(ctx, kPqCols, ncols * N * 32, &cols);  // wires, z, PI
    if (rc == KZG_OK) rc = ctx->pq_ws.get(ctx, kPqOut, N * 32, &d_out);
    if (rc == KZG_OK && !device) rc = ctx->pq_ws.get(ctx, kPqCoef, (N - n) * 32, &coef);
    if (rc == KZG_OK) rc = ctx->pq_ws.get(ctx, kPqFlag, 4, &flag);
    if (rc == KZG_OK && ((gate && !device) || lookup || custom)) rc = ctx->pq_ws.get(ctx, kPqGate, N * 32, &d_gate);
    if (rc) return rc;
    uint32_t *d_w = (uint32_t*)cols, *d_z = d_w + 8 * t * N, *d_pi = pi ? d_z + 8 * N : nullptr;
    uint32_t *d_m = d_w + 8 * nbase * N, *d_phi = d_m + 8 * N;  // (with a lookup record)
    if (round && lookup) {  // the resident coefficients [ f | PI | z | phi | m ] in one batched extension, in their own order
        d_pi = pi ? d_w + 8 * t * N : nullptr;
        d_z = d_w + 8 * (nbase - 1) * N;
        d_phi = d_w + 8 * nbase * N;
        d_m = d_phi + 8 * N;
        rc = pq_extend(ctx, s.stream, round->coef, n, n, -1, ncols, sh.lg_N, d_w, w, nullptr, true);
    } else if (round) {  // from the resident coefficients [ f | PI | z ]
        rc = pq_extend(ctx, s.stream, round->coef, n, n, -1, t, sh.lg_N, d_w, w, nullptr, true);
        if (rc == KZG_OK) rc = pq_extend(ctx, s.stream, round->coef + 8 * (ncols - 1) * n, n, n, -1, 1, sh.lg_N, d_z, w);
        if (rc == KZG_OK && pi) rc = pq_extend(ctx, s.stream, round->coef + 8 * t * n, n, n, -1, 1, sh.lg_N, d_pi, w);
    } else if (device) {
        rc = pq_extend(ctx, s.stream, (const uint32_t*)wires, stride, n, (int)sh.lg_n, t, sh.lg_N, d_w, w);
        if (rc == KZG_OK) rc = pq_extend(ctx, s.stream, (const uint32_t*)z, n, n, (int)sh.lg_n, 1, sh.lg_N, d_z, w);
        if (rc == KZG_OK && pi) rc = pq_extend(ctx, s.stream, (const uint32_t*)pi, n, n, (int)sh.lg_n, 1, sh.lg_N, d_pi, w);
        if (rc == KZG_OK && lookup) rc = pq_extend(ctx, s.stream, (const uint32_t*)lookup->mult, n, n, (int)sh.lg_n, 1, sh.lg_N, d_m, w);
        if (rc == KZG_OK && lookup) rc = pq_extend(ctx, s.stream, (const uint32_t*)lookup->phi, n, n, (int)sh.lg_n, 1, sh.lg_N, d_phi, w);
    } else {
        PqStaged src;  // [ wires | z | PI | m | phi ], as the extended columns: one extension
        rc = pq_stage(ctx, lk, s.stream, false, (uint32_t*)in, wires, stride, z, pi, n, t, false, &src);
        if (rc == KZG_OK && lookup) rc = pq_upload(ctx, lk, s.stream, (uint32_t*)in + 8 * nbase * n, (const uint64_t*)lookup->mult, n, 1, n);
        if (rc == KZG_OK && lookup)
            rc = pq_upload(ctx, lk, s.stream, (uint32_t*)in + 8 * (nbase + 1) * n, (const uint64_t*)lookup->phi, n, 1, n);
        if (rc == KZG_OK && gate) rc = pq_upload(ctx, lk, s.stream, (uint32_t*)d_gate, (const uint64_t*)gate, N, 1, N);
        if (rc == KZG_OK) rc = pq_extend(ctx, s.stream, src.w, n, n, (int)sh.lg_n, ncols, sh.lg_N, d_w, w);
    }
    if (rc == KZG_OK && lookup) {  // G' into the gate's workspace
        const LkKernelScalars lsc(lookup->theta, beta, alpha, c->c_tab);
        const uint32_t* key = c->coset.dev() + 8 * (2 * t + 2) * N;
        const LkColumns lc{d_w, key, key + 8 * c->c_tab * N, c->l0.dev(), d_m, d_phi};
        launch_lk_constraints(s.stream, lc, sh.lg_N, (uint32_t)sh.rot, (uint32_t)c->c_tab, N, lsc.view(), (uint32_t*)d_gate);
        HIP_TRY(ctx, hipGetLastError());
    }
    if (rc == KZG_OK && custom) rc = cg_enqueue(ctx, s.stream, c, sh, d_w, (uint32_t*)d_gate);
    if (rc == KZG_OK) rc = ck_constraints(ctx, s.stream, c, sh, d_w, d_z, d_pi, (const uint32_t*)d_gate, alpha, beta, gamma, (uint32_t*)d_out);
    bool remainder = false;
    if (rc == KZG_OK)
        rc = pq_finish(ctx, lk, s.stream, sh, (uint32_t*)d_out, false, w, (uint32_t*)coef, (uint32_t*)flag, 0, N - n,
                       device ? nullptr : out_coeffs, "circuit quotient", &remainder);
    if (rc) return rc;
    if (remainder) return pq_remainder(ctx, sh);
    if (!out_p1s) return KZG_OK;
    return pq_commit_chunks(ctx, lk, call.slot(), (const uint32_t*)coef, n, sh.rot - 1, out_p1s);
}

int kzg_circuit_quotient(kzg_ctx* ctx, const kzg_circuit* circuit, const uint64_t* wires, size_t stride, const uint64_t* z,
                         const uint64_t* public_inputs, const uint64_t alpha[4], const uint64_t beta[4], const uint64_t gamma[4],
                         const uint64_t* gate_coset, uint64_t* out_coeffs, uint64_t* out_p1s) {
    if (!ctx || !circuit || !wires || !z || !alpha || !beta || !gamma) return KZG_ERR_INVALID_ARG;
    if (ctx->multi) {
        kzg_ctx* kid = whole_srs_kid(ctx, out_p1s != nullptr, "the quotient's commitments need");
        if (!kid) return KZG_ERR_INVALID_ARG;
        return forwarded(ctx, kid, kzg_circuit_quotient(kid, circuit, wires, stride, z, public_inputs, alpha, beta, gamma, gate_coset,
                                                       out_coeffs, out_p1s));
    }
    return circuit_quotient_impl(ctx, circuit, wires, stride, z, public_inputs, alpha, beta, gamma, gate_coset, out_coeffs, out_p1s, false);
}

int kzg_circuit_quotient_device(kzg_ctx* ctx, const kzg_circuit* circuit, const void* d_wires, size_t stride, const void* d_z,
                                const void* d_public_inputs, const uint64_t alpha[4], const uint64_t beta[4], const uint64_t gamma[4],
                                const void* d_gate_coset, void* d_out_coeffs) {
    KZG_SINGLE_DEVICE_ONLY(ctx);
    if (!ctx || !circuit || !d_wires || !d_z || !alpha || !beta || !gamma || !d_out_coeffs) return KZG_ERR_INVALID_ARG;
    return circuit_quotient_impl(ctx, circuit, d_wires, stride, d_z, d_public_inputs, alpha, beta, gamma, d_gate_coset, d_out_coeffs,
                                 nullptr, true);
}

// ---- the lookup argument of a circuit whose key holds a table (lookup_circuit_kernels.hip) ---------------
// The per-proof columns: the folded columns f and T (k_lk_fold), the multiplicities of f in T and the running sum phi, by the
// kernels of section 4.21 on the call's own slot.  The call holds quotient_mu (the circuit), then lookup_mu (the hash table), then
// the context's mutex and one slot.
int kzg_circuit_lookup_columns(kzg_ctx* ctx, const kzg_circuit* circuit, const uint64_t* wires, size_t stride, const uint64_t theta[4],
                               const uint64_t beta[4], uint64_t* out_f, uint64_t* out_table, uint64_t* out_mult, uint64_t* out_phi,
                               uint64_t out_last[4], size_t* bad_row) {
    if (bad_row) *bad_row = (size_t)-1;
    if (!ctx || !circuit || !wires || !theta || !beta || !out_mult || !out_phi || !out_last) return KZG_ERR_INVALID_ARG;
    if (ctx->multi) {  // needs no SRS
        kzg_ctx* kid = multi_kid(ctx->multi, 0);
        return forwarded(ctx, kid, kzg_circuit_lookup_columns(kid, circuit, wires, stride, theta, beta, out_f, out_table, out_mult,
                                                             out_phi, out_last, bad_row));
    }
    // lookup_mu is taken after quotient_mu and given up after the frame has drained the stream (declared first, destroyed last)
    std::unique_lock<std::mutex> lkl(ctx->lookup_mu, std::defer_lock);
    PqCall call(ctx);
    if (!circuit_alive(ctx, circuit)) return circuit_foreign(ctx);
    const size_t n = circuit->n, t = circuit->t, c = circuit->c_tab;
    if (!c) {
        ctx->last_error = "circuit lookup columns: the circuit was created without a lookup table";
        return KZG_ERR_INVALID_ARG;
    }
    if (stride < n) return KZG_ERR_INVALID_ARG;
    lkl.lock();
    call.lock();
    int rc = call.begin();
    if (rc) return rc;
    std::unique_lock<std::mutex>& lk = call.lk();
    Slot& s = call.s();
    void* in = nullptr;
    rc = ctx->pq_ws.get(ctx, kPqIn, (c + 4) * n * 32, &in);  // [ the first c wires | f | T | m | phi ]
    if (rc == KZG_OK) rc = s.gp_flags.reserve(ctx, 64);
    if (rc) return rc;
    uint32_t *d_w = (uint32_t*)in, *d_f = d_w + 8 * c * n, *d_t = d_f + 8 * n, *d_m = d_t + 8 * n, *d_phi = d_m + 8 * n;
    rc = pq_upload(ctx, lk, s.stream, d_w, wires, n, c, stride);
    if (rc) return rc;
    const LkKernelScalars sc(theta, beta, nullptr, c);
    const uint32_t* tab = circuit->values.dev() + 8 * (2 * t + 2) * n;
    launch_lk_fold(s.stream, d_w, n, tab, tab + 8 * c * n, (uint32_t)n, (uint32_t)c, sc.view(), d_f, d_t);
    HIP_TRY(ctx, hipGetLastError());
    rc = lu_mult_enqueue(ctx, s, d_t, n, d_f, n, 1, n, lu_default_log_capacity(n), d_m, nullptr);
    if (rc == KZG_OK && out_f) rc = copy_unlocked(ctx, lk, s.stream, out_f, d_f, n * 32, hipMemcpyDeviceToHost, "hipMemcpyAsync (f)");
    if (rc == KZG_OK && out_table)
        rc = copy_unlocked(ctx, lk, s.stream, out_table, d_t, n * 32, hipMemcpyDeviceToHost, "hipMemcpyAsync (table)");
    if (rc == KZG_OK) rc = copy_unlocked(ctx, lk, s.stream, out_mult, d_m, n * 32, hipMemcpyDeviceToHost, "hipMemcpyAsync (multiplicities)");
    if (rc == KZG_OK) rc = sync_unlocked(ctx, lk, s.stream, "circuit lookup columns");
    if (rc == KZG_OK) rc = lu_mult_verdict(ctx, s, bad_row);
    if (rc) return rc;
    rc = run_on_slot(ctx, lk, s, RunCall{kLuLookupForm, d_f, nullptr, d_t, d_m, beta, n, 1, n}, d_phi, out_last, bad_row);
    if (rc) return rc;
    rc = copy_unlocked(ctx, lk, s.stream, out_phi, d_phi, n * 32, hipMemcpyDeviceToHost, "hipMemcpyAsync (phi)");
    return rc ? rc : sync_unlocked(ctx, lk, s.stream, "circuit lookup columns");
}

int kzg_circuit_lookup_quotient(kzg_ctx* ctx, const kzg_circuit* circuit, const uint64_t* wires, size_t stride, const uint64_t* z,
                                const uint64_t* mult, const uint64_t* phi, const uint64_t* public_inputs, const uint64_t alpha[4],
                                const uint64_t beta[4], const uint64_t gamma[4], const uint64_t theta[4], uint64_t* out_coeffs,
                                uint64_t* out_p1s) {
    if (!ctx || !circuit || !wires || !z || !mult || !phi || !alpha || !beta || !gamma || !theta) return KZG_ERR_INVALID_ARG;
    if (ctx->multi) {
        kzg_ctx* kid = whole_srs_kid(ctx, out_p1s != nullptr, "the quotient's commitments need");
        if (!kid) return KZG_ERR_INVALID_ARG;
        return forwarded(ctx, kid, kzg_circuit_lookup_quotient(kid, circuit, wires, stride, z, mult, phi, public_inputs, alpha, beta, gamma,
                                                              theta, out_coeffs, out_p1s));
    }
    const LookupRecord rec{mult, phi, theta};
    return circuit_quotient_impl(ctx, circuit, wires, stride, z, public_inputs, alpha, beta, gamma, nullptr, out_coeffs, out_p1s, false,
                                 nullptr, &rec);
}

// ---- zero-knowledge blinding of a circuit's proof (blind_kernels.hip) -------------------------------------
// f~ = f + b (X^n - 1): the values over H do not change, so z, the gate and the permutation are computed as before; in coefficient
// form the blinder is a patch (k_blind_patch).  The calls hold quotient_mu, then the context's mutex and one slot, as above.
namespace {
constexpr size_t kBlindWireLen = 2, kBlindZLen = 3;
// the blinder array of a circuit: t pairs for the wires, three for z, e - 2 for the chunks of T
size_t blind_count(size_t t, size_t e) { return 2 * t + kBlindZLen + (e - 2); }
// N >= t n + t + 4: T~ (degree t n + t + 2) fits and at least one coefficient is left that must vanish
bool blind_shape_ok(size_t n, size_t t, size_t e) { return e >= 2 && e * n >= t * n + t + 4; }
size_t blind_quotient_len(size_t n, size_t t, size_t e) { return (e - 1) * n + t + 3; }
// With custom gates of degree d_max (section 4.27) G'~ has degree n - 1 + d_max (n + 1) and T~ the degree
// max(t n + t + 2, d_max (n + 1) - 1); this many coefficients, which is the rule above's t n + t + 3 for d_max <= t (d_max = 0: none)
size_t blind_quotient_keep(size_t n, size_t t, size_t d_max) {
    const size_t base = t * n + t + 3, cust = d_max * (n + 1);
    return cust > base ? cust : base;
}
// ... they have to fit T~'s L_T coefficients, and N has to leave at least one coefficient that must vanish
bool blind_custom_shape_ok(size_t n, size_t t, size_t e, size_t d_max) {
    const size_t keep = blind_quotient_keep(n, t, d_max);
    return blind_shape_ok(n, t, e) && keep <= blind_quotient_len(n, t, e) && e * n >= keep + 1;
}
bool blind_values_ok(kzg_ctx* ctx, const char* what, const uint64_t* blinders, size_t count, std::vector<hf::Fr>* out) {
    out->resize(count);
    for (size_t i = 0; i < count; i++)
        if (!fr_arg_below_r(blinders + 4 * i, &(*out)[i])) {
            ctx->last_error = std::string(what) + ": blinder " + std::to_string(i) + " is not below r";
            return false;
        }
    return true;
}
int blind_shape_refused(kzg_ctx* ctx, const char* what) {
    ctx->last_error = std::string(what) + ": the blinded quotient needs 2^log_ext n >= t n + t + 4";
    return KZG_ERR_INVALID_ARG;
}
int blind_custom_shape_refused(kzg_ctx* ctx, const char* what) {
    ctx->last_error = std::string(what) + ": the blinded quotient of custom gates of degree d needs max(t n + t + 3, d (n + 1)) "
                      "<= (2^log_ext - 1) n + t + 3 and < 2^log_ext n";
    return KZG_ERR_INVALID_ARG;
}
// A blinded lookup proof (section 4.30): phi~ = phi + p Z_H with three blinders (linearised at zeta and opened at zeta w, like z),
// m~ = m + u Z_H with two.  The array is section 4.24's with p_0 .. p_2 and u_0, u_1 behind it.
constexpr size_t kBlindPhiLen = 3, kBlindMultLen = 2;
size_t lookup_blind_count(size_t t, size_t e) { return blind_count(t, e) + kBlindPhiLen + kBlindMultLen; }
// deg Lk1 = deg (phi~(w X) - phi~) F~ Tt = (n + 2) + 2 n + (n - 1) = 4 n + 1, so T~ has max(t n + t + 3, 3 n + 2) coefficients
size_t lookup_blind_keep(size_t n, size_t t) {
    const size_t base = t * n + t + 3, look = 3 * n + 2;
    return look > base ? look : base;
}
bool lookup_blind_shape_ok(size_t n, size_t t, size_t e, size_t c) {
    const size_t keep = lookup_blind_keep(n, t);
    return lookup_shape_ok(t, e, c) && keep < e * n && keep <= blind_quotient_len(n, t, e);
}
int lookup_blind_shape_refused(kzg_ctx* ctx, const char* what) {
    ctx->last_error = std::string(what) + ": the blinded lookup quotient needs max(t n + t + 3, 3 n + 2) <= (2^log_ext - 1) n + t + 3 "
                      "and < 2^log_ext n";
    return KZG_ERR_INVALID_ARG;
}
// `count` values uniform below r by rejection: r has 255 bits, a draw is kept with probability 0.906
int blind_draw(size_t count, uint64_t* out) {
    for (size_t i = 0; i < count; i++) {
        hf::Fr v;
        do {
            if (!vc_random(v.l, 32)) return KZG_ERR_HIP;
            v.l[3] &= 0x7fffffffffffffffULL;
        } while (hf::fr_geq(v, hf::kFrMod));
        std::memcpy(out + 4 * i, v.l, 32);
    }
    return KZG_OK;
}
}  // namespace

int kzg_circuit_lookup_blinded_sizes(size_t n, size_t t, unsigned log_ext, size_t c, size_t* num_blinders, size_t* quotient_len) {
    PqShape sh;
    if (log_ext > kPqMaxLogExt || !pq_shape(n, (size_t)1 << log_ext, &sh) || t < KZG_CIRCUIT_MIN_COLUMNS || t > kPqMaxColumns ||
        !lookup_blind_shape_ok(n, t, sh.rot, c))
        return KZG_ERR_INVALID_ARG;
    if (num_blinders) *num_blinders = lookup_blind_count(t, sh.rot);
    if (quotient_len) *quotient_len = blind_quotient_len(n, t, sh.rot);
    return KZG_OK;
}

int kzg_circuit_lookup_blinders(size_t t, unsigned log_ext, uint64_t* out) {
    if (!out || t < KZG_CIRCUIT_MIN_COLUMNS || t > kPqMaxColumns || log_ext > kPqMaxLogExt || !lookup_shape_ok(t, (size_t)1 << log_ext, 1))
        return KZG_ERR_INVALID_ARG;
    return blind_draw(lookup_blind_count(t, (size_t)1 << log_ext), out);
}

int kzg_circuit_custom_blinded_sizes(size_t n, size_t t, unsigned log_ext, size_t d_max, size_t* num_blinders, size_t* quotient_len) {
    PqShape sh;
    if (log_ext > kPqMaxLogExt || !pq_shape(n, (size_t)1 << log_ext, &sh) || t < KZG_CIRCUIT_MIN_COLUMNS || t > kPqMaxColumns ||
        t + 1 > sh.rot || d_max < 1 || d_max + 1 > sh.rot || !blind_custom_shape_ok(n, t, sh.rot, d_max))
        return KZG_ERR_INVALID_ARG;
    if (num_blinders) *num_blinders = blind_count(t, sh.rot);
    if (quotient_len) *quotient_len = blind_quotient_len(n, t, sh.rot);
    return KZG_OK;
}

int kzg_circuit_blinded_sizes(size_t n, size_t t, unsigned log_ext, size_t* num_blinders, size_t* quotient_len) {
    PqShape sh;
    if (log_ext > kPqMaxLogExt || !pq_shape(n, (size_t)1 << log_ext, &sh) || t < KZG_CIRCUIT_MIN_COLUMNS || t > kPqMaxColumns ||
        t + 1 > sh.rot || !blind_shape_ok(n, t, sh.rot))
        return KZG_ERR_INVALID_ARG;
    if (num_blinders) *num_blinders = blind_count(t, sh.rot);
    if (quotient_len) *quotient_len = blind_quotient_len(n, t, sh.rot);
    return KZG_OK;
}

int kzg_circuit_blinders(size_t t, unsigned log_ext, uint64_t* out) {
    if (!out || t < KZG_CIRCUIT_MIN_COLUMNS || t > kPqMaxColumns || log_ext > kPqMaxLogExt || t + 1 > ((size_t)1 << log_ext))
        return KZG_ERR_INVALID_ARG;
    return blind_draw(blind_count(t, (size_t)1 << log_ext), out);
}

// evals: k columns of n values over H (host); the k x (n + nb) blinded coefficients go to out_coeffs (host, column c at + 4 c
// out_stride u64, or null) and their commitments to out_p1s (or null)
static int blind_evaluations_impl(kzg_ctx* ctx, const char* what, const uint64_t* evals, size_t n, size_t k, size_t stride,
                                  const uint64_t* blinders, size_t nb, uint64_t* out_coeffs, size_t out_stride, uint64_t* out_p1s) {
    uint32_t lg_n = 0;
    if (!ntt_log(n, &lg_n) || k < 1 || k > kMaxCoefficients || stride < n || nb < 1 || nb > kBlindLow || (out_coeffs && out_stride < n + nb))
        return KZG_ERR_INVALID_ARG;
    const size_t len = n + nb;
    PqCall call(ctx);
    std::vector<hf::Fr> bl;
    if (!blind_values_ok(ctx, what, blinders, k * nb, &bl)) return KZG_ERR_INVALID_ARG;
    call.lock();
    int rc = pq_srs_status(ctx, out_p1s != nullptr, len);
    if (rc == KZG_OK) rc = call.begin();
    if (rc) return rc;
    std::unique_lock<std::mutex>& lk = call.lk();
    Slot& s = call.s();
    PqBufs w;
    void *in, *stack, *d_bl;
    rc = pq_bufs(ctx, n, 1, &w);
    if (rc == KZG_OK) rc = ctx->pq_ws.get(ctx, kPqIn, k * n * 32, &in);
    if (rc == KZG_OK) rc = ctx->pq_ws.get(ctx, kPqBlind, k * len * 32, &stack);
    if (rc == KZG_OK) rc = ctx->pq_ws.get(ctx, kPqChunks, k * nb * 32, &d_bl);
    if (rc) return rc;
    uint32_t *d_in = (uint32_t*)in, *d_c = (uint32_t*)stack;
    rc = pq_upload(ctx, lk, s.stream, d_in, evals, n, k, stride);
    if (rc == KZG_OK) rc = copy_unlocked(ctx, lk, s.stream, d_bl, blinders, k * nb * 32, hipMemcpyHostToDevice, "hipMemcpyAsync (blinders)");
    if (rc) return rc;
    const Fr30* itw = (const Fr30*)ctx->ntt_tw.p + 2 * kNttTableLen;
    const Fr30 inv_n = fr30_arg_from_mont256(hf::fr_inv(fr_pow2(lg_n)));
    for (size_t b = 0; b < k; b++) launch_ntt(s.stream, d_in + 8 * b * n, d_c + 8 * b * len, lg_n, itw, inv_n, w.A, w.B);
    launch_blind_patch(s.stream, d_c, (uint32_t)n, k, len, (const uint32_t*)d_bl, (const uint32_t*)d_bl, (uint32_t)nb, k);
    HIP_TRY(ctx, hipGetLastError());
    if (out_coeffs) {
        lk.unlock();
        const hipError_t e = hipMemcpy2DAsync(out_coeffs, out_stride * 32, d_c, len * 32, len * 32, k, hipMemcpyDeviceToHost, s.stream);
        lk.lock();
        if (e != hipSuccess) return hip_fail(ctx, "hipMemcpy2DAsync (blinded coefficients)", e);
    }
    rc = sync_unlocked(ctx, lk, s.stream, what);
    if (rc || !out_p1s) return rc;
    return pq_commit_chunks(ctx, lk, call.slot(), d_c, len, k, out_p1s);
}

int kzg_blind_evaluations(kzg_ctx* ctx, const uint64_t* evals, size_t n, size_t k, size_t stride, const uint64_t* blinders, size_t nb,
                          uint64_t* out_coeffs, size_t out_stride) {
    if (!ctx || !evals || !blinders || !out_coeffs) return KZG_ERR_INVALID_ARG;
    if (ctx->multi) {  // needs no SRS
        kzg_ctx* kid = multi_kid(ctx->multi, 0);
        return forwarded(ctx, kid, kzg_blind_evaluations(kid, evals, n, k, stride, blinders, nb, out_coeffs, out_stride));
    }
    return blind_evaluations_impl(ctx, "blind evaluations", evals, n, k, stride, blinders, nb, out_coeffs, out_stride, nullptr);
}

int kzg_commit_evaluations_blinded(kzg_ctx* ctx, const uint64_t* evals, size_t n, size_t k, size_t stride, const uint64_t* blinders,
                                   size_t nb, uint64_t* out_p1s) {
    if (!ctx || !evals || !blinders || !out_p1s) return KZG_ERR_INVALID_ARG;
    if (ctx->multi) {
        kzg_ctx* kid = whole_srs_kid(ctx, true, "the blinded commitments need");
        if (!kid) return KZG_ERR_INVALID_ARG;
        return forwarded(ctx, kid, kzg_commit_evaluations_blinded(kid, evals, n, k, stride, blinders, nb, out_p1s));
    }
    return blind_evaluations_impl(ctx, "commit evaluations (blinded)", evals, n, k, stride, blinders, nb, nullptr, 0, out_p1s);
}

// wires (t columns of n values), z and pi (n values or null) are host pointers, or device pointers when `device`; then out_coeffs
// (L_T coefficients) is a device pointer.  out_p1s: host, or null.  With a lookup record (section 4.30; host pointers, or a round
// of the prover, and no custom record) m and phi are transformed back, patched and extended with the wires and z -- the stack is
// [ f_0 .. f_(t-1) | m | z | phi ], so that the two patches only widen by a column -- and k_lk_constraints fills the gate's workspace
static int circuit_quotient_blinded_impl(kzg_ctx* ctx, const kzg_circuit* c, const void* wires, size_t stride, const void* z,
                                         const void* pi, const uint64_t* alpha, const uint64_t* beta, const uint64_t* gamma,
                                         const uint64_t* blinders, void* out_coeffs, uint64_t* out_p1s, bool device,
                                         const ProveRound* round = nullptr, const CustomRecord* custom = nullptr,
                                         const LookupRecord* lookup = nullptr) {
    PqCall call(ctx, round);
    if (!circuit_alive(ctx, c)) return circuit_foreign(ctx);
    PqShape sh;
    if (!pq_shape(c->n, (size_t)1 << c->lg_ext, &sh) || stride < c->n) return KZG_ERR_INVALID_ARG;
    if (lookup && !c->c_tab) {
        ctx->last_error = "circuit lookup quotient (blinded): the circuit was created without a lookup table";
        return KZG_ERR_INVALID_ARG;
    }
    if (lookup && (custom || (device && !round))) return KZG_ERR_INVALID_ARG;
    const size_t n = sh.n, N = sh.N, t = c->t, e = sh.rot, nbase = t + 1 + (pi ? 1 : 0), nlk = lookup ? 1 : 0, ncols = nbase + 2 * nlk,
                 nstack = t + 1 + 2 * nlk;
    if (lookup && !lookup_blind_shape_ok(n, t, e, c->c_tab)) return lookup_blind_shape_refused(ctx, "circuit lookup quotient (blinded)");
    if (!blind_shape_ok(n, t, e)) return blind_shape_refused(ctx, "circuit quotient (blinded)");
    if (custom && !c->g_custom) return custom_refused(ctx, "circuit custom quotient (blinded)");
    if (custom && (custom->rho || c->rho)) return custom_kind_refused(ctx, "circuit custom quotient (blinded)", false);
    if (custom && !blind_custom_shape_ok(n, t, e, custom->d_max)) return blind_custom_shape_refused(ctx, "circuit custom quotient (blinded)");
    std::vector<hf::Fr> bl;
    const size_t nbl = lookup ? lookup_blind_count(t, e) : blind_count(t, e);
    if (!blind_values_ok(ctx, lookup ? "circuit lookup quotient (blinded)" : "circuit quotient (blinded)", blinders, nbl, &bl))
        return KZG_ERR_INVALID_ARG;
    const size_t LT = blind_quotient_len(n, t, e), clen = n + kBlindZLen, Lc = n + t + 3,
                 keep = lookup ? lookup_blind_keep(n, t) : blind_quotient_keep(n, t, custom ? custom->d_max : 0);
    if (device) {
        const size_t ob = LT * 32;
        if (pq_overlap(out_coeffs, ob, wires, ((t - 1) * stride + n) * 32) || pq_overlap(out_coeffs, ob, z, n * 32) ||
            (pi && pq_overlap(out_coeffs, ob, pi, n * 32))) {
            ctx->last_error = "circuit quotient (blinded): the output overlaps an input";
            return KZG_ERR_INVALID_ARG;
        }
    }
    call.lock();
    int rc = pq_srs_status(ctx, out_p1s != nullptr, Lc);
    if (rc == KZG_OK) rc = call.begin();
    if (rc) return rc;
    std::unique_lock<std::mutex>& lk = call.lk();
    Slot& s = call.s();
    PqBufs w;
    void *in = nullptr, *cols, *d_out, *coef = out_coeffs, *flag, *stack, *chunks, *d_gate = nullptr;
    // the blinders as the patches read them: the array as given, then a zero and the chunk blinders once more ([0, d_0 .. d_(e-3)]
    // are the low blinders of the e - 1 chunks, [d_0 ..] the high ones)
    // With a lookup record the array's groups lie in the stack's order: [ b | u | c | p | d ], then the zero and the d once more.
    const size_t bl_words = 8 * (nbl + 1 + (e - 2)), zcol = t + nlk, bl_z = 2 * t + kBlindMultLen * nlk;
    rc = pq_bufs(ctx, N, ncols, &w);
    if (rc == KZG_OK && !device) rc = ctx->pq_ws.get(ctx, kPqIn, ncols * n * 32, &in);
    if (rc == KZG_OK) rc = ctx->pq_ws.get(ctx, kPqCols, ncols * N * 32, &cols);  // wires, z, PI on the coset
    if (rc == KZG_OK) rc = ctx->pq_ws.get(ctx, kPqOut, N * 32, &d_out);
    if (rc == KZG_OK && !device) rc = ctx->pq_ws.get(ctx, kPqCoef, LT * 32, &coef);
    if (rc == KZG_OK) rc = ctx->pq_ws.get(ctx, kPqFlag, 4, &flag);
    if (rc == KZG_OK) rc = ctx->pq_ws.get(ctx, kPqBlind, nstack * clen * 32 + bl_words * 4, &stack);  // the blinded coefficients
    if (rc == KZG_OK && out_p1s) rc = ctx->pq_ws.get(ctx, kPqChunks, (e - 1) * Lc * 32, &chunks);
    if (rc == KZG_OK && (custom || lookup)) rc = ctx->pq_ws.get(ctx, kPqGate, N * 32, &d_gate);
    if (rc) return rc;
    // on the coset: [ f | z | PI ], with a lookup record [ f | m | z | phi | PI ]
    uint32_t *d_w = (uint32_t*)cols, *d_z = d_w + 8 * zcol * N, *d_pi = pi ? d_w + 8 * nstack * N : nullptr;
    uint32_t *d_m = d_w + 8 * t * N, *d_phi = d_z + 8 * N;  // (with a lookup record)
    uint32_t *d_c = (uint32_t*)stack, *d_bl = d_c + 8 * nstack * clen;
    {
        std::vector<uint64_t> hb(bl_words / 2, 0);
        const uint64_t* d_src = blinders + 4 * (2 * t + kBlindZLen);  // d_0 .. d_(e-3)
        if (lookup) {
            const uint64_t *p_src = d_src + 4 * (e - 2), *u_src = p_src + 4 * kBlindPhiLen;
            std::memcpy(hb.data(), blinders, 2 * t * 32);
            std::memcpy(hb.data() + 4 * 2 * t, u_src, kBlindMultLen * 32);
            std::memcpy(hb.data() + 4 * bl_z, blinders + 4 * 2 * t, kBlindZLen * 32);
            std::memcpy(hb.data() + 4 * (bl_z + kBlindZLen), p_src, kBlindPhiLen * 32);
        } else {
            std::memcpy(hb.data(), blinders, nbl * 32);
        }
        std::memcpy(hb.data() + 4 * (nbl + 1), d_src, (e - 2) * 32);
        rc = copy_unlocked(ctx, lk, s.stream, d_bl, hb.data(), bl_words * 4, hipMemcpyHostToDevice, "hipMemcpyAsync (blinders)");
        if (rc == KZG_OK) rc = sync_unlocked(ctx, lk, s.stream, "circuit quotient (blinded)");  // (hb leaves scope)
        if (rc) return rc;
    }
    PqStaged src;
    rc = pq_stage(ctx, lk, s.stream, device, (uint32_t*)in, wires, stride, z, pi, n, t, false, &src);
    if (rc == KZG_OK && lookup && !round) {  // [ wires | z | PI | m | phi ] in the staging buffer
        rc = pq_upload(ctx, lk, s.stream, (uint32_t*)in + 8 * nbase * n, (const uint64_t*)lookup->mult, n, 1, n);
        if (rc == KZG_OK) rc = pq_upload(ctx, lk, s.stream, (uint32_t*)in + 8 * (nbase + 1) * n, (const uint64_t*)lookup->phi, n, 1, n);
    }
    if (rc) return rc;
    {  // the wires and z (m and phi with them): values -> coefficients -> patch -> the coset, from n + 3 coefficients each
        const Fr30* itw = (const Fr30*)ctx->ntt_tw.p + 2 * kNttTableLen;
        const Fr30 inv_n = fr30_arg_from_mont256(hf::fr_inv(fr_pow2(sh.lg_n)));
        if (round) {  // the resident coefficients [ f | PI | z ] (a lookup round: [ f | PI | z | phi | m ]), copied under the patches
            const uint32_t* u_z = round->coef + 8 * (nbase - 1) * n;
            HIP_TRY(ctx, hipMemcpy2DAsync(d_c, clen * 32, round->coef, n * 32, n * 32, t, hipMemcpyDeviceToDevice, s.stream));
            if (lookup) {
                HIP_TRY(ctx, hipMemcpyAsync(d_c + 8 * t * clen, u_z + 16 * n, n * 32, hipMemcpyDeviceToDevice, s.stream));
                HIP_TRY(ctx, hipMemcpy2DAsync(d_c + 8 * zcol * clen, clen * 32, u_z, n * 32, n * 32, 2, hipMemcpyDeviceToDevice, s.stream));
            } else {
                HIP_TRY(ctx, hipMemcpyAsync(d_c + 8 * t * clen, u_z, n * 32, hipMemcpyDeviceToDevice, s.stream));
            }
        } else {
            for (size_t j = 0; j < t; j++) launch_ntt(s.stream, src.w + 8 * j * src.stride, d_c + 8 * j * clen, sh.lg_n, itw, inv_n, w.A, w.B);
            launch_ntt(s.stream, src.z, d_c + 8 * zcol * clen, sh.lg_n, itw, inv_n, w.A, w.B);
            if (lookup) {
                const uint32_t* s_m = (const uint32_t*)in + 8 * nbase * n;
                launch_ntt(s.stream, s_m, d_c + 8 * t * clen, sh.lg_n, itw, inv_n, w.A, w.B);
                launch_ntt(s.stream, s_m + 8 * n, d_c + 8 * (zcol + 1) * clen, sh.lg_n, itw, inv_n, w.A, w.B);
            }
        }
        // nb = 2: the wires (and m behind them); nb = 3: z (and phi behind it)
        launch_blind_patch(s.stream, d_c, (uint32_t)n, zcol, clen, d_bl, d_bl, kBlindWireLen, zcol);
        launch_blind_patch(s.stream, d_c + 8 * zcol * clen, (uint32_t)n, 1 + nlk, clen, d_bl + 8 * bl_z, d_bl + 8 * bl_z, kBlindZLen, 1 + nlk);
        HIP_TRY(ctx, hipGetLastError());
        rc = pq_extend(ctx, s.stream, d_c, clen, clen, -1, nstack, sh.lg_N, d_w, w, nullptr, round != nullptr);
        if (rc == KZG_OK && pi && round) rc = pq_extend(ctx, s.stream, round->coef + 8 * t * n, n, n, -1, 1, sh.lg_N, d_pi, w);
        if (rc == KZG_OK && pi && !round) rc = pq_extend(ctx, s.stream, src.pi, n, n, (int)sh.lg_n, 1, sh.lg_N, d_pi, w);
        if (rc) return rc;
    }
    if (custom) {  // G'~ from the blinded wires on the coset
        rc = cg_enqueue(ctx, s.stream, c, sh, d_w, (uint32_t*)d_gate);
        if (rc) return rc;
    }
    if (lookup) {  // G'~ = alpha^3 Lk1 + alpha^4 Lk2 from the blinded columns on the coset
        const LkKernelScalars lsc(lookup->theta, beta, alpha, c->c_tab);
        const uint32_t* key = c->coset.dev() + 8 * (2 * t + 2) * N;
        const LkColumns lc{d_w, key, key + 8 * c->c_tab * N, c->l0.dev(), d_m, d_phi};
        launch_lk_constraints(s.stream, lc, sh.lg_N, (uint32_t)sh.rot, (uint32_t)c->c_tab, N, lsc.view(), (uint32_t*)d_gate);
        HIP_TRY(ctx, hipGetLastError());
    }
    rc = ck_constraints(ctx, s.stream, c, sh, d_w, d_z, d_pi, (const uint32_t*)d_gate, alpha, beta, gamma, (uint32_t*)d_out);
    if (rc) return rc;
    // T~ has t n + t + 3 coefficients (with custom gates of a degree above t: d_max (n + 1); with a lookup record max(t n + t + 3,
    // 3 n + 2)): those are kept, whatever follows up to N must vanish, and up to L_T the output is zero
    if (LT > keep) HIP_TRY(ctx, hipMemsetAsync((uint32_t*)coef + 8 * keep, 0, (LT - keep) * 32, s.stream));
    bool remainder = false;
    rc = pq_finish(ctx, lk, s.stream, sh, (uint32_t*)d_out, false, w, (uint32_t*)coef, (uint32_t*)flag, keep, LT,
                   device ? nullptr : out_coeffs, "circuit quotient (blinded)", &remainder);
    if (rc) return rc;
    if (remainder) {
        ctx->last_error = "quotient: the blinded numerator is not divisible by X^" + std::to_string(n) +
                          " - 1 (a coefficient of the interpolant at [" + std::to_string(keep) + ", N) is not zero): the constraints do not hold on the domain";
        return KZG_ERR_REMAINDER;
    }
    if (!out_p1s) return KZG_OK;
    // the chunks T~_c = T_c + d_c X^n - d_(c-1), each padded to n + t + 3 coefficients; the last one keeps its own top
    uint32_t* d_ch = (uint32_t*)chunks;
    const uint32_t* d_t = (const uint32_t*)coef;
    if (e > 2) HIP_TRY(ctx, hipMemcpy2DAsync(d_ch, Lc * 32, d_t, n * 32, n * 32, e - 2, hipMemcpyDeviceToDevice, s.stream));
    HIP_TRY(ctx, hipMemcpyAsync(d_ch + 8 * (e - 2) * Lc, d_t + 8 * (e - 2) * n, Lc * 32, hipMemcpyDeviceToDevice, s.stream));
    if (e > 2) launch_blind_patch(s.stream, d_ch, (uint32_t)n, e - 1, Lc, d_bl + 8 * nbl, d_bl + 8 * (nbl + 1), 1, e - 2);
    HIP_TRY(ctx, hipGetLastError());
    return pq_commit_chunks(ctx, lk, call.slot(), d_ch, Lc, e - 1, out_p1s);  // (checks the SRS again: the waits dropped the mutex)
}

int kzg_circuit_quotient_blinded(kzg_ctx* ctx, const kzg_circuit* circuit, const uint64_t* wires, size_t stride, const uint64_t* z,
                                 const uint64_t* public_inputs, const uint64_t alpha[4], const uint64_t beta[4], const uint64_t gamma[4],
                                 const uint64_t* blinders, uint64_t* out_coeffs, uint64_t* out_p1s) {
    if (!ctx || !circuit || !wires || !z || !alpha || !beta || !gamma || !blinders) return KZG_ERR_INVALID_ARG;
    if (ctx->multi) {
        kzg_ctx* kid = whole_srs_kid(ctx, out_p1s != nullptr, "the quotient's commitments need");
        if (!kid) return KZG_ERR_INVALID_ARG;
        return forwarded(ctx, kid, kzg_circuit_quotient_blinded(kid, circuit, wires, stride, z, public_inputs, alpha, beta, gamma, blinders,
                                                               out_coeffs, out_p1s));
    }
    return circuit_quotient_blinded_impl(ctx, circuit, wires, stride, z, public_inputs, alpha, beta, gamma, blinders, out_coeffs, out_p1s,
                                         false);
}

int kzg_circuit_quotient_blinded_device(kzg_ctx* ctx, const kzg_circuit* circuit, const void* d_wires, size_t stride, const void* d_z,
                                        const void* d_public_inputs, const uint64_t alpha[4], const uint64_t beta[4],
                                        const uint64_t gamma[4], const uint64_t* blinders, void* d_out_coeffs, uint64_t* out_p1s) {
    KZG_SINGLE_DEVICE_ONLY(ctx);
    if (!ctx || !circuit || !d_wires || !d_z || !alpha || !beta || !gamma || !blinders || !d_out_coeffs) return KZG_ERR_INVALID_ARG;
    return circuit_quotient_blinded_impl(ctx, circuit, d_wires, stride, d_z, d_public_inputs, alpha, beta, gamma, blinders, d_out_coeffs,
                                         out_p1s, true);
}

int kzg_circuit_lookup_quotient_blinded(kzg_ctx* ctx, const kzg_circuit* circuit, const uint64_t* wires, size_t stride, const uint64_t* z,
                                        const uint64_t* mult, const uint64_t* phi, const uint64_t* public_inputs, const uint64_t alpha[4],
                                        const uint64_t beta[4], const uint64_t gamma[4], const uint64_t theta[4], const uint64_t* blinders,
                                        uint64_t* out_coeffs, uint64_t* out_p1s) {
    if (!ctx || !circuit || !wires || !z || !mult || !phi || !alpha || !beta || !gamma || !theta || !blinders) return KZG_ERR_INVALID_ARG;
    if (ctx->multi) {
        kzg_ctx* kid = whole_srs_kid(ctx, out_p1s != nullptr, "the quotient's commitments need");
        if (!kid) return KZG_ERR_INVALID_ARG;
        return forwarded(ctx, kid, kzg_circuit_lookup_quotient_blinded(kid, circuit, wires, stride, z, mult, phi, public_inputs, alpha, beta,
                                                                      gamma, theta, blinders, out_coeffs, out_p1s));
    }
    const LookupRecord rec{mult, phi, theta};
    return circuit_quotient_blinded_impl(ctx, circuit, wires, stride, z, public_inputs, alpha, beta, gamma, blinders, out_coeffs, out_p1s,
                                         false, nullptr, nullptr, &rec);
}

// ---- the custom gates of a circuit whose key holds selector x monomial terms (custom_gate_kernels.hip) -----
static CustomRecord custom_record(const kzg_circuit* c) {
    return CustomRecord{c->g_custom, c->d_max, c->exps, c->rho, c->exps_next, c->next_wires};
}

// The test hook of k_cg_gate: the wires to the coset as the quotient extends them, G' on it, N values to the host.  Needs no SRS.
// (next: kzg_circuit_custom_next_gate, the test hook of k_cgn_gate, on a next-row handle only; else on a custom handle only)
static int custom_gate_impl(kzg_ctx* ctx, const kzg_circuit* circuit, const uint64_t* wires, size_t stride, uint64_t* out_gate_coset,
                            bool next) {
    if (!ctx || !circuit || !wires || !out_gate_coset) return KZG_ERR_INVALID_ARG;
    if (ctx->multi) {
        kzg_ctx* kid = multi_kid(ctx->multi, 0);
        return forwarded(ctx, kid, custom_gate_impl(kid, circuit, wires, stride, out_gate_coset, next));
    }
    PqCall call(ctx);
    if (!circuit_alive(ctx, circuit)) return circuit_foreign(ctx);
    if (!circuit->g_custom) return custom_refused(ctx, "circuit custom gate");
    if (next != (circuit->rho != 0)) return custom_kind_refused(ctx, "circuit custom gate", next);
    PqShape sh;
    if (!pq_shape(circuit->n, (size_t)1 << circuit->lg_ext, &sh) || stride < circuit->n) return KZG_ERR_INVALID_ARG;
    const size_t n = sh.n, N = sh.N, t = circuit->t;
    call.lock();
    int rc = call.begin();
    if (rc) return rc;
    std::unique_lock<std::mutex>& lk = call.lk();
    Slot& s = call.s();
    PqBufs w;
    void *in, *cols, *d_gate;
    rc = pq_bufs(ctx, N, t, &w);
    if (rc == KZG_OK) rc = ctx->pq_ws.get(ctx, kPqIn, t * n * 32, &in);
    if (rc == KZG_OK) rc = ctx->pq_ws.get(ctx, kPqCols, t * N * 32, &cols);
    if (rc == KZG_OK) rc = ctx->pq_ws.get(ctx, kPqGate, N * 32, &d_gate);
    if (rc) return rc;
    rc = pq_upload(ctx, lk, s.stream, (uint32_t*)in, wires, n, t, stride);
    if (rc == KZG_OK) rc = pq_extend(ctx, s.stream, (const uint32_t*)in, n, n, (int)sh.lg_n, t, sh.lg_N, (uint32_t*)cols, w);
    if (rc == KZG_OK) rc = cg_enqueue(ctx, s.stream, circuit, sh, (const uint32_t*)cols, (uint32_t*)d_gate);
    if (rc == KZG_OK) rc = copy_unlocked(ctx, lk, s.stream, out_gate_coset, d_gate, N * 32, hipMemcpyDeviceToHost, "hipMemcpyAsync (custom gate)");
    return rc ? rc : sync_unlocked(ctx, lk, s.stream, "circuit custom gate");
}
int kzg_circuit_custom_gate(kzg_ctx* ctx, const kzg_circuit* circuit, const uint64_t* wires, size_t stride, uint64_t* out_gate_coset) {
    return custom_gate_impl(ctx, circuit, wires, stride, out_gate_coset, false);
}
int kzg_circuit_custom_next_gate(kzg_ctx* ctx, const kzg_circuit* circuit, const uint64_t* wires, size_t stride, uint64_t* out_gate_coset) {
    return custom_gate_impl(ctx, circuit, wires, stride, out_gate_coset, true);
}

// (next: kzg_circuit_custom_next_quotient, never blinded, on a next-row handle only; else on a custom handle only)
static int custom_quotient_impl(kzg_ctx* ctx, const kzg_circuit* circuit, const uint64_t* wires, size_t stride, const uint64_t* z,
                                const uint64_t* public_inputs, const uint64_t alpha[4], const uint64_t beta[4], const uint64_t gamma[4],
                                const uint64_t* blinders, uint64_t* out_coeffs, uint64_t* out_p1s, bool next) {
    if (!ctx || !circuit || !wires || !z || !alpha || !beta || !gamma) return KZG_ERR_INVALID_ARG;
    if (ctx->multi) {
        kzg_ctx* kid = whole_srs_kid(ctx, out_p1s != nullptr, "the quotient's commitments need");
        if (!kid) return KZG_ERR_INVALID_ARG;
        return forwarded(ctx, kid, custom_quotient_impl(kid, circuit, wires, stride, z, public_inputs, alpha, beta, gamma, blinders, out_coeffs,
                                                       out_p1s, next));
    }
    CustomRecord rec{};
    {  // the record is the circuit's: read under quotient_mu, as the bodies read it again
        std::lock_guard<std::mutex> lkq(ctx->quotient_mu);
        if (!circuit_alive(ctx, circuit)) return circuit_foreign(ctx);
        if (!circuit->g_custom) return custom_refused(ctx, "circuit custom quotient");
        if (next != (circuit->rho != 0)) return custom_kind_refused(ctx, "circuit custom quotient", next);
        rec = custom_record(circuit);
    }
    if (blinders)
        return circuit_quotient_blinded_impl(ctx, circuit, wires, stride, z, public_inputs, alpha, beta, gamma, blinders, out_coeffs, out_p1s,
                                             false, nullptr, &rec);
    return circuit_quotient_impl(ctx, circuit, wires, stride, z, public_inputs, alpha, beta, gamma, nullptr, out_coeffs, out_p1s, false,
                                 nullptr, nullptr, &rec);
}
int kzg_circuit_custom_quotient(kzg_ctx* ctx, const kzg_circuit* circuit, const uint64_t* wires, size_t stride, const uint64_t* z,
                                const uint64_t* public_inputs, const uint64_t alpha[4], const uint64_t beta[4], const uint64_t gamma[4],
                                const uint64_t* blinders, uint64_t* out_coeffs, uint64_t* out_p1s) {
    return custom_quotient_impl(ctx, circuit, wires, stride, z, public_inputs, alpha, beta, gamma, blinders, out_coeffs, out_p1s, false);
}
int kzg_circuit_custom_next_quotient(kzg_ctx* ctx, const kzg_circuit* circuit, const uint64_t* wires, size_t stride, const uint64_t* z,
                                     const uint64_t* public_inputs, const uint64_t alpha[4], const uint64_t beta[4],
                                     const uint64_t gamma[4], uint64_t* out_coeffs, uint64_t* out_p1s) {
    return custom_quotient_impl(ctx, circuit, wires, stride, z, public_inputs, alpha, beta, gamma, nullptr, out_coeffs, out_p1s, true);
}

// ---- the last round of a circuit's proof: linearise, open once (linearise_kernels.hip) --------------------
// The calls hold quotient_mu, then the context's mutex and one slot, as the quotient's calls above: the per-proof coefficients live
// in pq_ws, the tables, the values and the G_p in the slot's buffers of the openings at several point sets.
namespace {
const hf::Fr kFrZero = {{0, 0, 0, 0}};
bool fr_equal(const hf::Fr& a, const hf::Fr& b) { return std::memcmp(a.l, b.l, 32) == 0; }

// r(X) = sum_k scalar_k C_k(X) + konst: its t + e + 3 columns where they lie on the device, with the scalars the evaluations give
struct LinTerm {
    const uint32_t* coeffs;
    hf::Fr scalar;
};
struct LinPoly {
    std::vector<LinTerm> terms;
    hf::Fr konst = kFrZero;
};
struct LinChallenges {
    hf::Fr alpha, beta, gamma, zeta;
};
// What the lookup adds to r (section 4.26): the scalars on phi(X) and m(X) and the constant, from the evaluations abar (the first
// c), tbar (c), qbar and phiw = phi(zeta w):
//     r_L = r + (alpha^4 l - alpha^3 F T) phi(X) + alpha^3 F m(X) + alpha^3 (phiw F T - T),  F = beta + qbar sum theta^j abar_j,
//     T = beta + sum theta^j tbar_j, l = L_0(zeta)
struct LookupLin {
    hf::Fr on_phi, on_m, konst;
};
LookupLin lookup_lin(size_t n, uint32_t lg_n, size_t c, const LinChallenges& ch, const hf::Fr& theta, const hf::Fr* abar,
                     const hf::Fr* tbar, const hf::Fr& qbar, const hf::Fr& phiw) {
    const hf::Fr Z = hf::fr_sub(hf::fr_pow(ch.zeta, n), hf::kFrOne), zm1 = hf::fr_sub(ch.zeta, hf::kFrOne);
    const hf::Fr l0 = fr_equal(zm1, kFrZero) ? hf::kFrOne : hf::fr_mul(Z, hf::fr_inv(hf::fr_mul(fr_pow2(lg_n), zm1)));
    hf::Fr fa = kFrZero, ft = kFrZero, p = hf::kFrOne;
    for (size_t j = 0; j < c; j++) {
        fa = hf::fr_add(fa, hf::fr_mul(p, abar[j]));
        ft = hf::fr_add(ft, hf::fr_mul(p, tbar[j]));
        p = hf::fr_mul(p, theta);
    }
    const hf::Fr F = hf::fr_add(ch.beta, hf::fr_mul(qbar, fa)), T = hf::fr_add(ch.beta, ft), FT = hf::fr_mul(F, T);
    const hf::Fr a3 = hf::fr_mul(hf::fr_mul(ch.alpha, ch.alpha), ch.alpha), a4 = hf::fr_mul(a3, ch.alpha);
    LookupLin out;
    out.on_phi = hf::fr_sub(hf::fr_mul(a4, l0), hf::fr_mul(a3, FT));
    out.on_m = hf::fr_mul(a3, F);
    out.konst = hf::fr_mul(a3, hf::fr_sub(hf::fr_mul(phiw, FT), T));
    return out;
}
// What the custom gates add to r (section 4.27): the g scalars prod_j abar_j^p[s][j], which the prover puts on the coefficients of
// the qx_s and the verifier on their commitments:  r_X = r + sum_s (prod_j abar_j^p[s][j]) qx_s(X)
// A next-row circuit (section 4.28; exps_next not null) has the scalars prod_j abar_j^p[s][j] abar'_j^p'[s][j] with abar'_j =
// f_j(zeta w): abar_next holds the rho values of the wires next_wires[0 .. rho), in that order.  One function for prover and verifier
void custom_lin_scalars(size_t t, size_t g, const uint8_t* exps, const hf::Fr* abar, std::vector<hf::Fr>* out,
                        const uint8_t* exps_next = nullptr, size_t rho = 0, const uint8_t* next_wires = nullptr,
                        const hf::Fr* abar_next = nullptr) {
    out->clear();
    for (size_t s = 0; s < g; s++) {
        hf::Fr m = hf::kFrOne;
        for (size_t j = 0; j < t; j++)
            for (unsigned k = 0; k < exps[s * t + j]; k++) m = hf::fr_mul(m, abar[j]);
        for (size_t i = 0; exps_next && i < rho; i++)
            for (unsigned k = 0; k < exps_next[s * t + next_wires[i]]; k++) m = hf::fr_mul(m, abar_next[i]);
        out->push_back(m);
    }
}
// The scalars of r, which the prover puts on coefficient vectors and the verifier on commitments, in the order q_0 .. q_(t-1),
// q_M, q_C, z, sigma_(t-1), T_0 .. T_(e-2); *konst: the constant term.  abar: t values, sbar: t - 1, zw = z(zeta w),
// pi_zeta = PI(zeta) (zero without public inputs); shifts: the t k_j
void lin_scalars(size_t n, uint32_t lg_n, size_t t, size_t e, const uint64_t* shifts, const LinChallenges& ch, const hf::Fr* abar,
                 const hf::Fr* sbar, const hf::Fr& zw, const hf::Fr& pi_zeta, std::vector<hf::Fr>* out, hf::Fr* konst) {
    const hf::Fr zn = hf::fr_pow(ch.zeta, n), Z = hf::fr_sub(zn, hf::kFrOne);
    // l = L_0(zeta), the polynomial's value: Z / (n (zeta - 1)) off zeta = 1 (zero elsewhere on H), and 1 at zeta = 1
    const hf::Fr zm1 = hf::fr_sub(ch.zeta, hf::kFrOne);
    const hf::Fr l0 = fr_equal(zm1, kFrZero) ? hf::kFrOne : hf::fr_mul(Z, hf::fr_inv(hf::fr_mul(fr_pow2(lg_n), zm1)));
    hf::Fr A = hf::kFrOne, B = zw;
    for (size_t j = 0; j < t; j++) {
        const hf::Fr ag = hf::fr_add(abar[j], ch.gamma);
        A = hf::fr_mul(A, hf::fr_add(ag, hf::fr_mul(hf::fr_mul(ch.beta, pq_fr(shifts + 4 * j)), ch.zeta)));
        if (j + 1 < t) B = hf::fr_mul(B, hf::fr_add(ag, hf::fr_mul(ch.beta, sbar[j])));
    }
    const hf::Fr a2l = hf::fr_mul(hf::fr_mul(ch.alpha, ch.alpha), l0), aB = hf::fr_mul(ch.alpha, B);
    std::vector<hf::Fr>& sc = *out;
    sc.assign(abar, abar + t);
    sc.push_back(hf::fr_mul(abar[0], abar[1]));
    sc.push_back(hf::kFrOne);
    sc.push_back(hf::fr_add(hf::fr_mul(ch.alpha, A), a2l));
    sc.push_back(hf::fr_sub(kFrZero, hf::fr_mul(aB, ch.beta)));
    hf::Fr zc = hf::fr_sub(kFrZero, Z);  // -Z zeta^(c n)
    for (size_t k = 0; k + 1 < e; k++) {
        sc.push_back(zc);
        zc = hf::fr_mul(zc, zn);
    }
    *konst = hf::fr_sub(hf::fr_sub(pi_zeta, hf::fr_mul(aB, hf::fr_add(abar[t - 1], ch.gamma))), a2l);
}
// key: the circuit's resident coefficients (2 t + 2 columns of n), d_z: z's coefficients, d_t: T's N - n coefficients
void lin_poly(const kzg_circuit* c, const LinChallenges& ch, const hf::Fr* abar, const hf::Fr* sbar, const hf::Fr& zw,
              const hf::Fr& pi_zeta, const uint32_t* key, const uint32_t* d_z, const uint32_t* d_t, LinPoly* out) {
    const size_t n = c->n, t = c->t, e = (size_t)1 << c->lg_ext;
    LinPoly& r = *out;
    std::vector<hf::Fr> sc;
    lin_scalars(n, c->lg_n, t, e, c->shifts, ch, abar, sbar, zw, pi_zeta, &sc, &r.konst);
    for (size_t j = 0; j < t + 2; j++) r.terms.push_back({key + 8 * j * n, sc[j]});
    r.terms.push_back({d_z, sc[t + 2]});
    r.terms.push_back({key + 8 * (2 * t + 1) * n, sc[t + 3]});  // sigma_(t-1)
    for (size_t k = 0; k + 1 < e; k++) r.terms.push_back({d_t + 8 * k * n, sc[t + 4 + k]});
}
LinColumn lin_column(const uint32_t* coeffs, const hf::Fr& mult) {
    LinColumn col = {};
    col.coeffs = coeffs;
    const Fr30 m = fr30_arg_from_mont256(mult);
    std::memcpy(col.mult, m.d, sizeof col.mult);
    return col;
}
int lin_remainder(kzg_ctx* ctx) {
    ctx->last_error = "circuit open: the linearisation polynomial does not vanish at zeta (r(zeta) != 0): T is not the quotient of "
                      "these wires and this z";
    return KZG_ERR_REMAINDER;
}

// The slot's table of a blinded round (s.btab): per distinct point the records of k_blind_tail and the t + 6 powers of the point,
// then the blinders as the records point at them, 32 bytes an entry: [b_j0, b_j1, 0] per wire, [c_0, c_1, c_2], and per chunk of T
// [d_(c-1), 0, 0, d_c] (d_(-1) = d_(e-2) = 0); in a lookup round (section 4.30) then [p_0, p_1, p_2] and [u_0, u_1, 0].
constexpr size_t kBlindPointBytes = 1536, kBlindValueBytes = 64 * 32;
static_assert(kBlindMaxColumns * sizeof(BlindColumn) + (kPqMaxColumns + 3 + kBlindLow) * sizeof(Fr30) <= kBlindPointBytes, "btab");
static_assert((3 * kPqMaxColumns + 3 + 4 * 7 + 3 + 3) * 32 <= kBlindValueBytes, "btab");
static_assert(kPqMaxColumns + 2 + 7 <= kBlindMaxColumns, "the wires, z twice (n = 1: one point) and the chunks of T");
// (a lookup round has phi~ and m~ as well: t + e + 2 records at zeta, within kBlindMaxColumns by the lookup's shape rule, t <= 6 and
// e <= 8, and not by this assertion; blind_tails counts before it writes)
// Behind the launches of k_lin_combine (G_p over [0, n) from the unblinded columns, at s.sg + 8 p L words): what the blinders add.
// lin: r~'s terms with the scalars of the blinded evaluations; d_t: T~'s coefficients, whose last chunk reaches to n + t + 3.
// phi_poly: the stack's index of phi~ in a lookup round (r~_L's terms then end with phi~ and m~: two more records at zeta and one
// at zeta w, t + e + 2 <= kBlindMaxColumns at zeta since the lookup's shape rule gives t <= 6 and e <= 8), or 0.
int blind_tails(kzg_ctx* ctx, Slot& s, const SetsPlan& plan, const LinPoly& lin, const std::vector<hf::Fr>& bl, const uint32_t* d_t,
                size_t n, size_t t, size_t e, uint32_t* d_y, size_t phi_poly = 0) {
    const size_t ntail = t + 3, L = n + ntail, val_off = kSetsMaxPoints * kBlindPointBytes, zb = 3 * t, cb = 3 * t + 3;
    const size_t pb = cb + 4 * (e - 1), ub = pb + 3;  // (a lookup round)
    uint8_t* h = (uint8_t*)s.btab.h;
    const uint8_t* d = (const uint8_t*)s.btab.d;
    uint64_t* hv = (uint64_t*)(h + val_off);
    const uint32_t* dv = (const uint32_t*)(d + val_off);
    std::memset(hv, 0, kBlindValueBytes);
    for (size_t j = 0; j < t; j++) {
        std::memcpy(hv + 4 * (3 * j), bl[2 * j].l, 32);
        std::memcpy(hv + 4 * (3 * j + 1), bl[2 * j + 1].l, 32);
    }
    for (size_t k = 0; k < kBlindZLen; k++) std::memcpy(hv + 4 * (zb + k), bl[2 * t + k].l, 32);
    const hf::Fr* dc = bl.data() + 2 * t + kBlindZLen;  // d_0 .. d_(e-3)
    for (size_t c = 0; c + 1 < e; c++) {
        if (c >= 1) std::memcpy(hv + 4 * (cb + 4 * c), dc[c - 1].l, 32);
        if (c + 2 < e) std::memcpy(hv + 4 * (cb + 4 * c + 3), dc[c].l, 32);
    }
    if (phi_poly) {  // p_0 .. p_2 and u_0, u_1 lie behind the d_c
        for (size_t k = 0; k < kBlindPhiLen; k++) std::memcpy(hv + 4 * (pb + k), dc[e - 2 + k].l, 32);
        for (size_t k = 0; k < kBlindMultLen; k++) std::memcpy(hv + 4 * (ub + k), dc[e - 2 + kBlindPhiLen + k].l, 32);
    }
    auto column = [&](size_t low_entry, const uint32_t* tail, size_t tail_len, const hf::Fr& mult) {
        BlindColumn col = {};
        col.tail = tail;
        col.low = dv + 8 * low_entry;
        const Fr30 m = fr30_arg_from_mont256(mult);
        std::memcpy(col.mult, m.d, sizeof col.mult);
        col.tail_len = (uint32_t)tail_len;
        return col;
    };
    uint32_t ncols[KZG_MAX_SET_POINTS];
    for (size_t p = 0; p < plan.npts; p++) {
        BlindColumn* out = (BlindColumn*)(h + p * kBlindPointBytes);
        uint32_t k = 0;
        for (uint32_t en = plan.off[p]; en < plan.off[p + 1]; en++) {
            const uint32_t i = plan.sel[en];
            const hf::Fr& m = plan.mult[en];
            // the records this polynomial adds, before any is written (cannot happen: without a lookup the static_assert above,
            // with one its shape rule -- t + e + 2 <= 16 at zeta, t + e + 4 = 14 at n = 1, where D < N leaves t = 2, e = 8 alone)
            const size_t adds = i == 0 ? e + (phi_poly ? 2 : 0) : (i <= t || i == 2 * t || (phi_poly && i == phi_poly) ? 1 : 0);
            if (k + adds > kBlindMaxColumns) return KZG_ERR_INVALID_ARG;
            if (i == 0) {  // r~: z~ and the chunks of T~ with r's scalars
                out[k++] = column(zb, dv + 8 * zb, kBlindZLen, hf::fr_mul(m, lin.terms[t + 2].scalar));
                for (size_t c = 0; c + 1 < e; c++) {
                    const hf::Fr sc = hf::fr_mul(m, lin.terms[t + 4 + c].scalar);
                    if (c + 2 < e) out[k++] = column(cb + 4 * c, dv + 8 * (cb + 4 * c + 3), 1, sc);
                    else out[k++] = column(cb + 4 * c, d_t + 8 * (e - 1) * n, ntail, sc);
                }
                if (phi_poly) {  // phi~ and m~ with r_L's scalars (lin's last two terms)
                    const size_t nt = lin.terms.size();
                    out[k++] = column(pb, dv + 8 * pb, kBlindPhiLen, hf::fr_mul(m, lin.terms[nt - 2].scalar));
                    out[k++] = column(ub, dv + 8 * ub, kBlindMultLen, hf::fr_mul(m, lin.terms[nt - 1].scalar));
                }
            } else if (i <= t) {
                out[k++] = column(3 * (i - 1), dv + 8 * 3 * (i - 1), kBlindWireLen, m);
            } else if (i == 2 * t) {
                out[k++] = column(zb, dv + 8 * zb, kBlindZLen, m);
            } else if (phi_poly && i == phi_poly) {
                out[k++] = column(pb, dv + 8 * pb, kBlindPhiLen, m);
            }  // (the sigmas and the table are the key's: not blinded)
        }
        ncols[p] = k;
        Fr30* pw = (Fr30*)(h + p * kBlindPointBytes + kBlindMaxColumns * sizeof(BlindColumn));
        hf::Fr cur = hf::fr_pow(plan.pts[p], n);
        for (size_t j = 0; j < ntail; j++) {
            pw[j] = fr30_arg_from_mont256(cur);
            cur = hf::fr_mul(cur, plan.pts[p]);
        }
        cur = hf::kFrOne;
        for (size_t i = 0; i < kBlindLow; i++) {
            pw[ntail + i] = fr30_arg_from_mont256(cur);
            cur = hf::fr_mul(cur, plan.pts[p]);
        }
    }
    HIP_TRY(ctx, hipMemcpyAsync(s.btab.d, s.btab.h, val_off + kBlindValueBytes, hipMemcpyHostToDevice, s.stream));
    for (size_t p = 0; p < plan.npts; p++)
        launch_blind_tail(s.stream, (const BlindColumn*)(d + p * kBlindPointBytes), ncols[p], (uint32_t)n, (uint32_t)ntail,
                          (const Fr30*)(d + p * kBlindPointBytes + kBlindMaxColumns * sizeof(BlindColumn)), s.sg.dev() + 8 * p * L,
                          d_y + 8 * p);
    HIP_TRY(ctx, hipGetLastError());
    return KZG_OK;
}
}  // namespace

// wires (t columns of n values), z, pi (n values or null) and t_coeffs (N - n coefficients) are host pointers, or device pointers
// when `device`.  v null: the test hook -- r's n coefficients to out_r, no SRS; else the proof to out_p1.
// blinders (host, or null; never with the test hook): the blinded round of DESIGN.md section 4.24 -- t_coeffs holds T~'s L_T
// coefficients, the evaluations are those of the blinded polynomials, every G_p has n + t + 3 coefficients: k_lin_combine sums
// [0, n) from the unblinded columns as before and k_blind_tail adds what the blinders change.
static int circuit_open_impl(kzg_ctx* ctx, const kzg_circuit* c, const void* wires, size_t stride, const void* z, const void* pi,
                             const void* t_coeffs, const uint64_t* alpha, const uint64_t* beta, const uint64_t* gamma,
                             const uint64_t* zeta, const uint64_t* v, uint64_t* out_evals, uint64_t* out_r, uint64_t* out_p1,
                             bool device, const uint64_t* blinders = nullptr, const ProveRound* round = nullptr,
                             const LookupRecord* lookup = nullptr, const CustomRecord* custom = nullptr) {
    PqCall call(ctx, round);
    if (!circuit_alive(ctx, c)) return circuit_foreign(ctx);
    PqShape sh;
    if (!pq_shape(c->n, (size_t)1 << c->lg_ext, &sh) || stride < c->n) return KZG_ERR_INVALID_ARG;
    if (lookup && (!c->c_tab || !round || !v)) return KZG_ERR_INVALID_ARG;  // (a round of kzg_circuit_lookup_prove or of its _blinded form only)
    if (custom && (!c->g_custom || !round || lookup || !v)) return KZG_ERR_INVALID_ARG;  // (a round of kzg_circuit_custom_prove only)
    if (custom && (custom->rho != c->rho || (custom->rho && (blinders || c->n < 2)))) return KZG_ERR_INVALID_ARG;
    // a next-row round (section 4.28): the rho wires of R are opened on {zeta, zeta w}; out_evals then has 2 t + rho values
    const size_t rho = custom ? custom->rho : 0;
    const size_t lc = lookup ? c->c_tab : 0;
    LinChallenges ch;
    hf::Fr vf = kFrZero;
    if (!fr_arg_below_r(alpha, &ch.alpha) || !fr_arg_below_r(beta, &ch.beta) || !fr_arg_below_r(gamma, &ch.gamma) ||
        !fr_arg_below_r(zeta, &ch.zeta) || (v && !fr_arg_below_r(v, &vf))) {
        ctx->last_error = "circuit open: a challenge is not below r";
        return KZG_ERR_INVALID_ARG;
    }
    const size_t n = sh.n, N = sh.N, t = c->t, npoly = 2 * t + 1 + (lookup ? lc + 2 : 0), ncoef = t + 1 + (pi ? 1 : 0);
    // blinded: every polynomial of the stack is padded to L = n + t + 3 coefficients, T~ has L_T of them
    const size_t e = sh.rot, ntail = blinders ? t + 3 : 0, L = n + ntail, t_len = blinders ? blind_quotient_len(n, t, e) : N - n;
    std::vector<hf::Fr> bl;
    if (blinders) {
        if (lookup && !lookup_blind_shape_ok(n, t, e, lc)) return lookup_blind_shape_refused(ctx, "circuit open (blinded)");
        if (!blind_shape_ok(n, t, e)) return blind_shape_refused(ctx, "circuit open (blinded)");
        if (custom && !blind_custom_shape_ok(n, t, e, custom->d_max)) return blind_custom_shape_refused(ctx, "circuit open (blinded)");
        if (!blind_values_ok(ctx, "circuit open (blinded)", blinders, lookup ? lookup_blind_count(t, e) : blind_count(t, e), &bl))
            return KZG_ERR_INVALID_ARG;
    }
    // the stack [ r | f_0 .. f_(t-1) | sigma_0 .. sigma_(t-2) | z ] on the sets {zeta}, {zeta w} (one point for n = 1, w = 1); with
    // a lookup record it goes on with [ tab_0 .. tab_(c-1) | q_K | phi ], phi in the second set
    const hf::Fr zeta_w = hf::fr_mul(ch.zeta, hf::fr_domain_root(sh.lg_n));
    // a next-row round: a third set {zeta, zeta w} for the wires of R -- still two distinct points, zeta the first of the plan
    std::vector<uint32_t> set_of(npoly, 0);
    set_of[2 * t] = 1;
    set_of[npoly - 1] = 1;
    std::vector<int> next_at(npoly, -1);  // polynomial i = 1 + j of the stack with j = R[k]: k
    for (size_t k = 0; k < rho; k++) {
        set_of[1 + custom->next_wires[k]] = 2;
        next_at[1 + custom->next_wires[k]] = (int)k;
    }
    const uint32_t set_len[3] = {1, 1, 2};
    const size_t nsets = rho ? 3 : 2;
    uint64_t zs[16];
    std::memcpy(zs, ch.zeta.l, 32);
    std::memcpy(zs + 4, zeta_w.l, 32);
    std::memcpy(zs + 8, zs, 64);
    SetsPlan plan;
    std::string why;
    if (!sets_plan(plan, why, npoly, set_of.data(), set_len, nsets, zs, vf.l)) {
        ctx->last_error = "circuit open: " + why;
        return KZG_ERR_INVALID_ARG;
    }
    call.lock();
    int rc = pq_srs_status(ctx, v != nullptr, L - 1);
    if (rc == KZG_OK) rc = call.begin();
    if (rc == KZG_OK) rc = pq_srs_status(ctx, v != nullptr, L - 1);  // (the wait for a slot dropped the mutex: the SRS may have changed)
    if (rc) return rc;
    std::unique_lock<std::mutex>& lk = call.lk();
    Slot& s = call.s();
    PqBufs w;
    void *in = nullptr, *stack, *scratch, *coef = const_cast<void*>(t_coeffs);
    rc = pq_bufs(ctx, n, 1, &w);
    if (rc == KZG_OK && !device) rc = ctx->pq_ws.get(ctx, kPqIn, ncoef * n * 32, &in);
    if (rc == KZG_OK) rc = ctx->pq_ws.get(ctx, kPqCols, ncoef * n * 32, &stack);  // the coefficients of the wires, PI, z
    if (rc == KZG_OK) rc = ctx->pq_ws.get(ctx, kPqOut, n * 32, &scratch);         // the passes' by-product; r for the test hook
    if (rc == KZG_OK && !device) rc = ctx->pq_ws.get(ctx, kPqCoef, t_len * 32, &coef);
    if (rc == KZG_OK) rc = sets_job_start(ctx, s, plan);
    if (rc == KZG_OK) rc = sets_ensure_all(ctx, s, plan, L, t + 1, 0);
    if (rc == KZG_OK) rc = s.ltab.reserve(ctx, kSetsMaxPoints * kLinMaxColumns * sizeof(LinColumn), s.stream);
    if (rc == KZG_OK && blinders) rc = s.btab.reserve(ctx, kSetsMaxPoints * kBlindPointBytes + kBlindValueBytes, s.stream);
    if (rc) return rc;
    // 1. coefficients: [ f_0 .. f_(t-1) | PI | z ], one inverse transform each
    uint32_t* d_f = round ? const_cast<uint32_t*>(round->coef) : (uint32_t*)stack;  // (a round's coefficients are only read)
    uint32_t *d_pi = pi ? d_f + 8 * t * n : nullptr, *d_z = d_f + 8 * (ncoef - 1) * n;
    if (!round) {
        PqStaged src;
        rc = pq_stage(ctx, lk, s.stream, device, (uint32_t*)in, wires, stride, z, pi, n, t, true, &src);
        if (rc == KZG_OK && !device) rc = pq_upload(ctx, lk, s.stream, (uint32_t*)coef, (const uint64_t*)t_coeffs, t_len, 1, t_len);
        if (rc) return rc;
        const Fr30* itw = (const Fr30*)ctx->ntt_tw.p + 2 * kNttTableLen;
        const Fr30 inv_n = fr30_arg_from_mont256(hf::fr_inv(fr_pow2(sh.lg_n)));
        for (size_t j = 0; j < t; j++) launch_ntt(s.stream, src.w + 8 * j * src.stride, d_f + 8 * j * n, sh.lg_n, itw, inv_n, w.A, w.B);
        if (pi) launch_ntt(s.stream, src.pi, d_pi, sh.lg_n, itw, inv_n, w.A, w.B);
        launch_ntt(s.stream, src.z, d_z, sh.lg_n, itw, inv_n, w.A, w.B);
        HIP_TRY(ctx, hipGetLastError());
    }
    // 2. evaluations, into the slot's value words: [0, t) the wires at zeta, [t] PI(zeta), [t + 1, 2 t) the sigmas, [2 t] z(zeta w)
    Fr30* tab = (Fr30*)s.stab.h;
    const Fr30* d_tab = (const Fr30*)s.stab.d;
    for (size_t r = 0; r < plan.npts; r++) combine_fill_powers(tab + r * kCombineTabGamma, plan.pts[r]);
    const size_t last_pt = plan.npts - 1;  // where zeta w sits
    for (size_t i = 0; i <= t + rho; i++) {  // the passes' own sums are not used: every weight is one
        tab[kSetsMultBase + i] = fr30_arg_from_mont256(hf::kFrOne);
        s.ssel.host()[i] = i <= t ? (uint32_t)i : (uint32_t)custom->next_wires[i - t - 1];  // (behind the identity: the wires of R)
    }
    HIP_TRY(ctx, hipMemcpyAsync(s.stab.d, s.stab.h, (kSetsMultBase + t + 1 + rho) * sizeof(Fr30), hipMemcpyHostToDevice, s.stream));
    HIP_TRY(ctx, hipMemcpyAsync(s.ssel.dev(), s.ssel.host(), (t + 1 + rho) * 4, hipMemcpyHostToDevice, s.stream));
    const uint32_t* key = c->coeffs.dev();
    uint32_t* d_vals = s.svals.dev();
    launch_sets_combine(s.stream, d_f, (uint32_t)n, (uint32_t)(ncoef - 1), n, d_tab, d_tab + kSetsMultBase, s.ssel.dev(), 0, false,
                        (uint32_t*)scratch, s.cpart.dev(), d_vals);
    launch_sets_combine(s.stream, key + 8 * (t + 2) * n, (uint32_t)n, (uint32_t)(t - 1), n, d_tab, d_tab + kSetsMultBase, s.ssel.dev(), 0,
                        false, (uint32_t*)scratch, s.cpart.dev(), d_vals + 8 * (t + 1));
    launch_sets_combine(s.stream, d_z, (uint32_t)n, 1, n, d_tab + last_pt * kCombineTabGamma, d_tab + kSetsMultBase, s.ssel.dev(), 0,
                        false, (uint32_t*)scratch, s.cpart.dev(), d_vals + 8 * 2 * t);
    const uint32_t *d_phi = d_z + 8 * n, *d_m = d_z + 16 * n;  // (a round with a lookup record: [ .. z | phi | m ])
    if (lookup) {  // [2 t + 1, 2 t + c] the table at zeta, [2 t + c + 1] q_K(zeta), [2 t + c + 2] phi(zeta w)
        launch_sets_combine(s.stream, key + 8 * (2 * t + 2) * n, (uint32_t)n, (uint32_t)(lc + 1), n, d_tab, d_tab + kSetsMultBase,
                            s.ssel.dev(), 0, false, (uint32_t*)scratch, s.cpart.dev(), d_vals + 8 * (2 * t + 1));
        launch_sets_combine(s.stream, d_phi, (uint32_t)n, 1, n, d_tab + last_pt * kCombineTabGamma, d_tab + kSetsMultBase, s.ssel.dev(), 0,
                            false, (uint32_t*)scratch, s.cpart.dev(), d_vals + 8 * (2 * t + 2 + lc));
    }
    if (rho)  // [npoly, npoly + rho) the wires of R at zeta w: one pass over the wires' coefficients, selected by the list of R
        launch_sets_combine(s.stream, d_f, (uint32_t)n, (uint32_t)rho, n, d_tab + last_pt * kCombineTabGamma, d_tab + kSetsMultBase + t + 1,
                            s.ssel.dev() + t + 1, 0, false, (uint32_t*)scratch, s.cpart.dev(), d_vals + 8 * npoly);
    HIP_TRY(ctx, hipGetLastError());
    rc = sync_unlocked(ctx, lk, s.stream, "circuit open (evaluations)");
    if (rc) return rc;
    std::vector<hf::Fr> ys(npoly, kFrZero);  // the stack's values: 0, abar, sbar, z(zeta w)
    std::vector<hf::Fr> ys_next(rho);        // ... and the second value of a wire of R, at zeta w: one value per (polynomial, point)
    const uint32_t* hv = s.svals.host();
    for (size_t k = 0; k < rho; k++) std::memcpy(ys_next[k].l, hv + 8 * (npoly + k), 32);
    for (size_t j = 0; j < t; j++) std::memcpy(ys[1 + j].l, hv + 8 * j, 32);
    for (size_t j = 0; j + 1 < t; j++) std::memcpy(ys[1 + t + j].l, hv + 8 * (t + 1 + j), 32);
    std::memcpy(ys[2 * t].l, hv + 8 * 2 * t, 32);
    for (size_t i = 2 * t + 1; i < npoly; i++) std::memcpy(ys[i].l, hv + 8 * i, 32);
    hf::Fr pi_zeta = kFrZero;
    if (pi) std::memcpy(pi_zeta.l, hv + 8 * t, 32);
    if (blinders) {  // f~_j(zeta) = f_j(zeta) + b_j(zeta) Z, z~(zeta w) = z(zeta w) + c(zeta w) Z: (zeta w)^n = zeta^n
        const hf::Fr Z = hf::fr_sub(hf::fr_pow(ch.zeta, n), hf::kFrOne);
        for (size_t j = 0; j < t; j++)
            ys[1 + j] = hf::fr_add(ys[1 + j], hf::fr_mul(hf::fr_add(bl[2 * j], hf::fr_mul(bl[2 * j + 1], ch.zeta)), Z));
        const hf::Fr* cz = &bl[2 * t];
        const hf::Fr cw = hf::fr_add(cz[0], hf::fr_mul(zeta_w, hf::fr_add(cz[1], hf::fr_mul(zeta_w, cz[2]))));
        ys[2 * t] = hf::fr_add(ys[2 * t], hf::fr_mul(cw, Z));
        if (lookup) {  // phi~(zeta w) = phi(zeta w) + p(zeta w) Z
            const hf::Fr* pz = &bl[2 * t + kBlindZLen + (e - 2)];
            const hf::Fr pw = hf::fr_add(pz[0], hf::fr_mul(zeta_w, hf::fr_add(pz[1], hf::fr_mul(zeta_w, pz[2]))));
            ys[npoly - 1] = hf::fr_add(ys[npoly - 1], hf::fr_mul(pw, Z));
        }
    }
    for (size_t i = 1; i < npoly; i++) std::memcpy(out_evals + 4 * (i - 1), ys[i].l, 32);
    for (size_t k = 0; k < rho; k++) std::memcpy(out_evals + 4 * (npoly - 1 + k), ys_next[k].l, 32);
    if (round && round->derive_v) {  // v is fixed after the evaluations: the plan's points, lists and sizes stay, its multipliers follow v
        uint64_t v_now[4];
        if (!round->derive_v(out_evals, v_now) || !fr_arg_below_r(v_now, &vf) ||
            !sets_plan(plan, why, npoly, set_of.data(), set_len, nsets, zs, vf.l))
            return KZG_ERR_INVALID_ARG;
    }
    LinPoly lin;
    lin_poly(c, ch, &ys[1], &ys[1 + t], ys[2 * t], pi_zeta, key, d_z, (const uint32_t*)coef, &lin);
    if (lookup) {  // r_L: two more terms and more of the constant
        const LookupLin ll = lookup_lin(n, sh.lg_n, lc, ch, pq_fr(lookup->theta), &ys[1], &ys[2 * t + 1], ys[2 * t + 1 + lc],
                                        ys[2 * t + 2 + lc]);
        lin.terms.push_back({d_phi, ll.on_phi});
        lin.terms.push_back({d_m, ll.on_m});
        lin.konst = hf::fr_add(lin.konst, ll.konst);
    }
    if (custom) {  // r_X: g more terms on the key's resident qx_s, behind every other term (blind_tails indexes the others)
        std::vector<hf::Fr> sc;
        custom_lin_scalars(t, c->g_custom, c->exps, &ys[1], &sc, rho ? c->exps_next : nullptr, rho, c->next_wires, ys_next.data());
        for (size_t k = 0; k < c->g_custom; k++) lin.terms.push_back({key + 8 * (2 * t + 2 + k) * n, sc[k]});
    }
    // 3. the sums.  Point p: G_p = sum_i mult_i P_i over the polynomials of the stack opened there, with m_0 r spread over r's
    // columns: one launch per point, r is never stored.  The test hook: r itself, with its bare scalars.
    LinColumn* cols = (LinColumn*)s.ltab.h;
    const LinColumn* d_cols = (const LinColumn*)s.ltab.d;
    auto lin_const = [](const hf::Fr& k) {
        LinConst out;
        std::memcpy(out.l, k.l, 32);
        return out;
    };
    uint32_t* d_y = d_vals + 8 * (npoly + rho);  // out(p) of point p at d_y + 8 p
    if (!v) {
        for (size_t k = 0; k < lin.terms.size(); k++) cols[k] = lin_column(lin.terms[k].coeffs, lin.terms[k].scalar);
        HIP_TRY(ctx, hipMemcpyAsync(s.ltab.d, s.ltab.h, lin.terms.size() * sizeof(LinColumn), hipMemcpyHostToDevice, s.stream));
        launch_lin_combine(s.stream, d_cols, (uint32_t)lin.terms.size(), (uint32_t)n, d_tab, lin_const(lin.konst), (uint32_t*)scratch,
                           s.cpart.dev(), d_y);
        HIP_TRY(ctx, hipGetLastError());
        rc = copy_unlocked(ctx, lk, s.stream, out_r, scratch, n * 32, hipMemcpyDeviceToHost, "hipMemcpyAsync (linearisation)");
        return rc ? rc : sync_unlocked(ctx, lk, s.stream, "circuit linearise");
    }
    hf::Fr want[KZG_MAX_SET_POINTS];  // sum_i mult_i y_i over the list of point p (r's value, zero, is what is proved)
    uint32_t ncols[KZG_MAX_SET_POINTS];
    LinConst konst[KZG_MAX_SET_POINTS];
    for (size_t p = 0; p < plan.npts; p++) {
        LinColumn* out = cols + p * kLinMaxColumns;
        uint32_t k = 0;
        hf::Fr kc = kFrZero;
        want[p] = kFrZero;
        for (uint32_t e = plan.off[p]; e < plan.off[p + 1]; e++) {
            const uint32_t i = plan.sel[e];
            const hf::Fr& m = plan.mult[e];
            // (point 0 is zeta, point 1 zeta w: a wire of R has a value at each)
            want[p] = hf::fr_add(want[p], hf::fr_mul(m, p == 1 && next_at[i] >= 0 ? ys_next[next_at[i]] : ys[i]));
            if (i == 0) {
                for (const LinTerm& term : lin.terms) out[k++] = lin_column(term.coeffs, hf::fr_mul(m, term.scalar));
                kc = hf::fr_mul(m, lin.konst);
            } else if (i <= t) {
                out[k++] = lin_column(d_f + 8 * (i - 1) * n, m);
            } else if (i < 2 * t) {
                out[k++] = lin_column(key + 8 * (t + 2 + (i - t - 1)) * n, m);
            } else if (i == 2 * t) {
                out[k++] = lin_column(d_z, m);
            } else if (i + 1 < npoly) {  // tab_j, q_K: the key's columns behind the sigmas
                out[k++] = lin_column(key + 8 * (2 * t + 2 + (i - 2 * t - 1)) * n, m);
            } else {
                out[k++] = lin_column(d_phi, m);
            }
        }
        // (3 t + e + 3 <= 32, with a lookup 3 t + e + c + 5 <= 32, with custom gates 3 t + e + 3 + g <= 32: cannot happen)
        if (k > kLinMaxColumns) return KZG_ERR_INVALID_ARG;
        ncols[p] = k;
        konst[p] = lin_const(kc);
    }
    HIP_TRY(ctx, hipMemcpyAsync(s.ltab.d, s.ltab.h, plan.npts * kLinMaxColumns * sizeof(LinColumn), hipMemcpyHostToDevice, s.stream));
    if (s.timing) HIP_TRY(ctx, hipEventRecord(s.cmb_ev[0], s.stream));
    for (size_t p = 0; p < plan.npts; p++)
        launch_lin_combine(s.stream, d_cols + p * kLinMaxColumns, ncols[p], (uint32_t)n, d_tab + p * kCombineTabGamma, konst[p],
                           s.sg.dev() + 8 * p * L, s.cpart.dev(), d_y + 8 * p);
    if (blinders) {
        rc = blind_tails(ctx, s, plan, lin, bl, (const uint32_t*)coef, n, t, e, d_y, lookup ? npoly - 1 : 0);
        if (rc) return rc;
    }
    if (s.timing) HIP_TRY(ctx, hipEventRecord(s.cmb_ev[1], s.stream));
    HIP_TRY(ctx, hipGetLastError());
    rc = sync_unlocked(ctx, lk, s.stream, "circuit open (sums)");
    if (rc) return rc;
    // G_zeta(zeta) = m_0 r(zeta) + sum_(i >= 1) mult_i y_i with m_0 = 1: r vanishes at zeta exactly when the two agree
    hf::Fr got;
    std::memcpy(got.l, hv + 8 * (npoly + rho), 32);
    if (!fr_equal(got, want[0])) return lin_remainder(ctx);
    // 4. the scans and the MSM of kzg_open_sets, unchanged
    rc = pq_srs_status(ctx, true, L - 1);  // (the waits dropped the mutex)
    if (rc == KZG_OK) rc = sets_enqueue_open(ctx, s, plan, L);
    if (rc) return rc;
    await_unlocked(lk, s);
    std::vector<uint64_t> unused(4 * plan.nvals);
    rc = wait_sets_locked(ctx, call.slot(), unused.data(), out_p1);
    s.kind = SLOT_RESERVED;  // (the mutex was held since the wait marked it idle)
    return rc;
}

// ORDER, for the three entry points below: the required pointers are checked BEFORE anything of *ctx is used but ctx->multi
// (read by KZG_SINGLE_DEVICE_ONLY) -- no lock, no last_error.  tests/test_circuit_open.py relies on it: it hands in a zeroed block as
// the context to see every NULL pointer refused without a device.
int kzg_circuit_open(kzg_ctx* ctx, const kzg_circuit* circuit, const uint64_t* wires, size_t stride, const uint64_t* z,
                     const uint64_t* public_inputs, const uint64_t* t_coeffs, const uint64_t alpha[4], const uint64_t beta[4],
                     const uint64_t gamma[4], const uint64_t zeta[4], const uint64_t v[4], uint64_t* out_evals, uint64_t out_p1[18]) {
    if (!ctx || !circuit || !wires || !z || !t_coeffs || !alpha || !beta || !gamma || !zeta || !v || !out_evals || !out_p1)
        return KZG_ERR_INVALID_ARG;
    if (ctx->multi) {
        kzg_ctx* kid = whole_srs_kid(ctx, true, "the opening needs");
        if (!kid) return KZG_ERR_INVALID_ARG;
        return forwarded(ctx, kid, kzg_circuit_open(kid, circuit, wires, stride, z, public_inputs, t_coeffs, alpha, beta, gamma, zeta, v,
                                                   out_evals, out_p1));
    }
    return circuit_open_impl(ctx, circuit, wires, stride, z, public_inputs, t_coeffs, alpha, beta, gamma, zeta, v, out_evals, nullptr,
                             out_p1, false);
}

int kzg_circuit_open_device(kzg_ctx* ctx, const kzg_circuit* circuit, const void* d_wires, size_t stride, const void* d_z,
                            const void* d_public_inputs, const void* d_t_coeffs, const uint64_t alpha[4], const uint64_t beta[4],
                            const uint64_t gamma[4], const uint64_t zeta[4], const uint64_t v[4], uint64_t* out_evals,
                            uint64_t out_p1[18]) {
    KZG_SINGLE_DEVICE_ONLY(ctx);
    if (!ctx || !circuit || !d_wires || !d_z || !d_t_coeffs || !alpha || !beta || !gamma || !zeta || !v || !out_evals || !out_p1)
        return KZG_ERR_INVALID_ARG;
    return circuit_open_impl(ctx, circuit, d_wires, stride, d_z, d_public_inputs, d_t_coeffs, alpha, beta, gamma, zeta, v, out_evals,
                             nullptr, out_p1, true);
}

int kzg_circuit_open_blinded(kzg_ctx* ctx, const kzg_circuit* circuit, const uint64_t* wires, size_t stride, const uint64_t* z,
                             const uint64_t* public_inputs, const uint64_t* t_coeffs, const uint64_t alpha[4], const uint64_t beta[4],
                             const uint64_t gamma[4], const uint64_t zeta[4], const uint64_t v[4], const uint64_t* blinders,
                             uint64_t* out_evals, uint64_t out_p1[18]) {
    if (!ctx || !circuit || !wires || !z || !t_coeffs || !alpha || !beta || !gamma || !zeta || !v || !blinders || !out_evals || !out_p1)
        return KZG_ERR_INVALID_ARG;
    if (ctx->multi) {
        kzg_ctx* kid = whole_srs_kid(ctx, true, "the opening needs");
        if (!kid) return KZG_ERR_INVALID_ARG;
        return forwarded(ctx, kid, kzg_circuit_open_blinded(kid, circuit, wires, stride, z, public_inputs, t_coeffs, alpha, beta, gamma,
                                                           zeta, v, blinders, out_evals, out_p1));
    }
    return circuit_open_impl(ctx, circuit, wires, stride, z, public_inputs, t_coeffs, alpha, beta, gamma, zeta, v, out_evals, nullptr,
                             out_p1, false, blinders);
}

int kzg_circuit_open_blinded_device(kzg_ctx* ctx, const kzg_circuit* circuit, const void* d_wires, size_t stride, const void* d_z,
                                    const void* d_public_inputs, const void* d_t_coeffs, const uint64_t alpha[4],
                                    const uint64_t beta[4], const uint64_t gamma[4], const uint64_t zeta[4], const uint64_t v[4],
                                    const uint64_t* blinders, uint64_t* out_evals, uint64_t out_p1[18]) {
    KZG_SINGLE_DEVICE_ONLY(ctx);
    if (!ctx || !circuit || !d_wires || !d_z || !d_t_coeffs || !alpha || !beta || !gamma || !zeta || !v || !blinders || !out_evals ||
        !out_p1)
        return KZG_ERR_INVALID_ARG;
    return circuit_open_impl(ctx, circuit, d_wires, stride, d_z, d_public_inputs, d_t_coeffs, alpha, beta, gamma, zeta, v, out_evals,
                             nullptr, out_p1, true, blinders);
}

int kzg_circuit_linearise(kzg_ctx* ctx, const kzg_circuit* circuit, const uint64_t* wires, size_t stride, const uint64_t* z,
                          const uint64_t* public_inputs, const uint64_t* t_coeffs, const uint64_t alpha[4], const uint64_t beta[4],
                          const uint64_t gamma[4], const uint64_t zeta[4], uint64_t* out_evals, uint64_t* out_r) {
    if (!ctx || !circuit || !wires || !z || !t_coeffs || !alpha || !beta || !gamma || !zeta || !out_evals || !out_r)
        return KZG_ERR_INVALID_ARG;
    if (ctx->multi) {  // needs no SRS
        kzg_ctx* kid = multi_kid(ctx->multi, 0);
        return forwarded(ctx, kid, kzg_circuit_linearise(kid, circuit, wires, stride, z, public_inputs, t_coeffs, alpha, beta, gamma, zeta,
                                                        out_evals, out_r));
    }
    return circuit_open_impl(ctx, circuit, wires, stride, z, public_inputs, t_coeffs, alpha, beta, gamma, zeta, nullptr, out_evals, out_r,
                             nullptr, false);
}

// weights: k blst_fr given by the caller (the test hook), or null for fresh random ones.  wire: the commitments, proofs and
// cells are its byte strings (section 4.12) and commitments_p1 / cells / proofs_p1 are null
static int verify_cells_impl(kzg_ctx* ctx, const uint64_t* commitments_p1, size_t num_commitments, const uint32_t* commitment_idx,
                             const uint32_t* cell_ids, const uint64_t* cells, const uint64_t* proofs_p1, size_t k,
                             unsigned log_domain, unsigned log_cell, const void* setup_g2, size_t g2_stride_bytes,
                             const uint64_t* weights, bool want_weights, uint64_t* out_lhs, uint64_t* out_rhs, int* valid,
                             const VcWire* wire = nullptr) {
    if (!ctx) return KZG_ERR_INVALID_ARG;
    auto invalid = [&](const std::string& why) {
        ctx->last_error = "verify cells: " + why;
        return KZG_ERR_INVALID_ARG;
    };
    CellsShape sh;
    if (!cells_shape(0, log_domain, log_cell, &sh)) return invalid("unsupported shape (log_domain, log_cell)");
    if (wire && wire->order != KZG_ORDER_NATURAL && wire->order != KZG_ORDER_BIT_REVERSED)
        return invalid("order is neither KZG_ORDER_NATURAL nor KZG_ORDER_BIT_REVERSED");
    if (k > KZG_VERIFY_MAX_CELLS) return invalid("more than KZG_VERIFY_MAX_CELLS records");
    if (num_commitments > KZG_VERIFY_MAX_CELLS) return invalid("more than KZG_VERIFY_MAX_CELLS commitments");
    const void* in_commitments = wire ? (const void*)wire->commitments48 : commitments_p1;
    const void* in_cells = wire ? (const void*)wire->values_be : cells;
    const void* in_proofs = wire ? (const void*)wire->proofs48 : proofs_p1;
    if (!valid || (want_weights && (!out_lhs || !out_rhs)) || (num_commitments && !in_commitments) ||
        (k && (!commitment_idx || !cell_ids || !in_cells || !in_proofs || !setup_g2 || (want_weights && !weights))))
        return invalid("a required pointer is NULL");
    if (!k) {
        if (want_weights) {
            const hf::P1 inf = hf::p1_inf();
            write_p1(out_lhs, inf);
            write_p1(out_rhs, inf);
        }
        *valid = 1;
        return KZG_OK;
    }
    for (size_t t = 0; t < k; t++) {
        if (commitment_idx[t] >= num_commitments)
            return invalid("record " + std::to_string(t) + ": commitment index " + std::to_string(commitment_idx[t]) +
                           " is not below num_commitments");
        if (cell_ids[t] >= sh.cells)
            return invalid("record " + std::to_string(t) + ": cell id " + std::to_string(cell_ids[t]) + " is not below N / l");
    }
    for (size_t t = 0; t < k && !wire; t++)  // (byte strings: the device's decoder checks them)
        for (size_t i = 0; i < sh.l; i++) {
            hf::Fr v;
            std::memcpy(v.l, cells + 4 * (t * sh.l + i), 32);
            if (hf::fr_geq(v, hf::kFrMod))
                return invalid("record " + std::to_string(t) + ": value " + std::to_string(i) + " is not below r");
        }
    hf::G2Affine g2[2];
    {
        const int rci = vc_check_inputs(ctx, "verify cells", want_weights ? weights : nullptr, proofs_p1, k, commitments_p1,
                                        num_commitments, setup_g2, g2_stride_bytes, sh.l, "l", g2, wire != nullptr);
        if (rci) return rci;
    }
    if (ctx->multi) {
        int rc = KZG_OK;
        kzg_ctx* kid = cells_kid(ctx, &rc);
        return kid ? forwarded(ctx, kid, verify_cells_impl(kid, commitments_p1, num_commitments, commitment_idx, cell_ids, cells,
                                                           proofs_p1, k, log_domain, log_cell, setup_g2, g2_stride_bytes, weights,
                                                           want_weights, out_lhs, out_rhs, valid, wire))
                   : rc;
    }
    VcBatch vb;
    vb.sh = &sh;
    vb.k = k;
    vb.B = num_commitments;
    vb.commitments = commitments_p1;
    vb.cells = cells;
    vb.proofs = proofs_p1;
    std::vector<uint32_t> own_ids;
    if (wire) {
        vb.wire_commitments = wire->commitments48;
        vb.wire_proofs = wire->proofs48;
        vb.wire_values = wire->values_be;
        vb.bit_reversed = wire->order == KZG_ORDER_BIT_REVERSED;
        if (vb.bit_reversed) {  // the sampling specs' cell c is this API's cell brp(c) over the N / l cells
            own_ids.resize(k);
            for (size_t t = 0; t < k; t++) own_ids[t] = wire_brp(cell_ids[t], sh.log_n - sh.log_l);
            cell_ids = own_ids.data();
        }
    }
    std::vector<hf::Fr> rho;
    {
        const int rcw = vc_weights(ctx, "verify cells", want_weights ? weights : nullptr, k, &rho, &vb.glv);
        if (rcw) return rcw;
    }
    // records sorted by cell id (counting sort), the distinct ids and their counts
    std::vector<uint32_t> count(sh.cells + 1, 0);
    for (size_t t = 0; t < k; t++) count[cell_ids[t] + 1]++;
    for (size_t j = 0; j < sh.cells; j++) {
        if (count[j + 1]) {
            vb.ids.push_back((uint32_t)j);
            vb.lens.push_back(count[j + 1]);
        }
        count[j + 1] += count[j];
    }
    vb.order.resize(k);
    for (size_t t = 0; t < k; t++) vb.order[count[cell_ids[t]]++] = (uint32_t)t;
    vb.rho30.resize(k);
    for (size_t t = 0; t < k; t++) vb.rho30[t] = fr30_arg_from_mont256(rho[vb.order[t]]);
    const hf::Fr zero = {{0, 0, 0, 0}};
    vb.U.assign(num_commitments, zero);
    for (size_t t = 0; t < k; t++) vb.U[commitment_idx[t]] = hf::fr_add(vb.U[commitment_idx[t]], rho[t]);
    uint64_t lhs[18], rhs[18];
    const int rc = vc_device(ctx, vb, lhs, rhs);
    if (rc) return rc;
    if (want_weights) {
        std::memcpy(out_lhs, lhs, sizeof lhs);
        std::memcpy(out_rhs, rhs, sizeof rhs);
    }
    *valid = vc_pair(lhs, rhs, g2[1], g2[0]);  // e(LHS, [s^l]G2) == e(RHS, G2)
    return KZG_OK;
}

int kzg_verify_cells_batch(kzg_ctx* ctx, const uint64_t* commitments_p1, size_t num_commitments, const uint32_t* commitment_idx,
                           const uint32_t* cell_ids, const uint64_t* cells, const uint64_t* proofs_p1, size_t k, unsigned log_domain,
                           unsigned log_cell, const void* setup_g2, size_t g2_stride_bytes, int* valid) {
    return verify_cells_impl(ctx, commitments_p1, num_commitments, commitment_idx, cell_ids, cells, proofs_p1, k, log_domain, log_cell,
                             setup_g2, g2_stride_bytes, nullptr, false, nullptr, nullptr, valid);
}

int kzg_verify_cells_lincomb(kzg_ctx* ctx, const uint64_t* commitments_p1, size_t num_commitments, const uint32_t* commitment_idx,
                             const uint32_t* cell_ids, const uint64_t* cells, const uint64_t* proofs_p1, size_t k,
                             unsigned log_domain, unsigned log_cell, const void* setup_g2, size_t g2_stride_bytes,
                             const uint64_t* weights, uint64_t out_lhs_p1[18], uint64_t out_rhs_p1[18], int* valid) {
    return verify_cells_impl(ctx, commitments_p1, num_commitments, commitment_idx, cell_ids, cells, proofs_p1, k, log_domain, log_cell,
                             setup_g2, g2_stride_bytes, weights, true, out_lhs_p1, out_rhs_p1, valid);
}

// ---- openings at arbitrary points: barycentric evaluation and one pairing for many openings (bary_kernels.hip, the kernels
// of verify_kernels.hip) ------------------------------------------------------------------------------
namespace {
constexpr size_t kBaryChunkValues = (size_t)1 << kNttMaxLog;  // values one pass of the evaluation stages in a slot, at most
constexpr size_t kBaryMinValues = 8;  // staging room per polynomial, in values: its partials, its point and its result fit
}  // namespace

// P_b(z_b) for every polynomial of the batch, in chunks through one slot's staging buffers.  d_ys (device, 8 words per
// polynomial) receives the values when given; out_ys (host) when given.  Validated arguments, single-device context.
// wire_be: the values are 32-byte big-endian strings at a stride of 32 x stride bytes per polynomial (evals null), decoded on
// the device through the kVcWire workspace -- the caller holds fk20_mu -- and read in bit-reversed order when asked; a value
// not below r is KZG_ERR_INVALID_ARG, named under `what`.
static int bary_host(kzg_ctx* ctx, const uint64_t* evals, uint32_t lg, size_t batch, size_t stride, const uint64_t* zs,
                     uint32_t* d_ys, uint64_t* out_ys, const uint8_t* wire_be = nullptr, bool bit_reversed = false,
                     const char* what = "evaluate evaluations") {
    const size_t n = (size_t)1 << lg;
    std::vector<Fr30> z30(batch);
    for (size_t b = 0; b < batch; b++) {
        hf::Fr z;
        std::memcpy(z.l, zs + 4 * b, 32);
        z30[b] = fr30_arg_from_mont256(z);
    }
    std::unique_lock<std::mutex> lk(ctx->mu);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    int rc = ensure_ntt(ctx);
    if (rc) return rc;
    const int slot = reserve_slot(ctx, lk, true);
    if (slot < 0) return KZG_ERR_BUSY;
    SlotLease lease{ctx, slot};
    Slot& s = ctx->slots[slot];
    const size_t per = std::max(n, kBaryMinValues);
    const size_t chunk = std::min(batch, std::max<size_t>(1, kBaryChunkValues / per));
    rc = ensure_slot_basics(ctx, s);
    if (rc == KZG_OK) rc = ensure_poly(ctx, s, chunk * per);
    void* wire = nullptr;  // a chunk's bytes, then the error word
    if (rc == KZG_OK && wire_be) rc = ctx->vc_ws.get(ctx, kVcWire, chunk * n * 32 + 16, &wire);
    if (rc) return rc;
    const uint32_t tiles = bary_tiles(lg);
    const Fr30 inv_n = fr30_arg_from_mont256(hf::fr_inv(fr_pow2(lg)));
    // q: [partials: chunk x tiles records | points: chunk Fr30 | results: chunk x 8 words]
    uint32_t* partial = s.q.dev();
    Fr30* dz = (Fr30*)(partial + chunk * tiles * kBaryPartialWords);
    uint32_t* res = (uint32_t*)(dz + chunk);
    res += (4 - ((res - s.q.dev()) & 3)) & 3;  // 16-byte aligned
    for (size_t b0 = 0; b0 < batch; b0 += chunk) {
        const size_t bc = std::min(chunk, batch - b0);
        uint32_t herr = 0xffffffffu;
        if (wire_be) {
            uint32_t* d_err = (uint32_t*)((char*)wire + chunk * n * 32);
            const uint8_t* src = wire_be + 32 * b0 * stride;
            if (stride == n || bc == 1) HIP_TRY(ctx, hipMemcpyAsync(wire, src, bc * n * 32, hipMemcpyHostToDevice, s.stream));
            else HIP_TRY(ctx, hipMemcpy2DAsync(wire, n * 32, src, stride * 32, n * 32, bc, hipMemcpyHostToDevice, s.stream));
            HIP_TRY(ctx, hipMemsetAsync(d_err, 0xff, 4, s.stream));
            launch_wire_fr(s.stream, wire, (uint32_t)(bc * n), lg, bit_reversed, s.stage.dev(), d_err);
            HIP_TRY(ctx, hipMemcpyAsync(&herr, d_err, 4, hipMemcpyDeviceToHost, s.stream));
        } else if (stride == n || bc == 1)
            HIP_TRY(ctx, hipMemcpyAsync(s.stage.dev(), evals + 4 * b0 * stride, bc * n * 32, hipMemcpyHostToDevice, s.stream));
        else
            HIP_TRY(ctx, hipMemcpy2DAsync(s.stage.dev(), n * 32, evals + 4 * b0 * stride, stride * 32, n * 32, bc, hipMemcpyHostToDevice,
                                          s.stream));
        HIP_TRY(ctx, hipMemcpyAsync(dz, z30.data() + b0, bc * sizeof(Fr30), hipMemcpyHostToDevice, s.stream));
        uint32_t* out = d_ys ? d_ys + 8 * b0 : res;
        launch_bary(s.stream, s.stage.dev(), lg, (uint32_t)bc, dz, ctx->ntt_tw.p, inv_n, partial, out);
        HIP_TRY(ctx, hipGetLastError());
        if (out_ys) HIP_TRY(ctx, hipMemcpyAsync(out_ys + 4 * b0, out, bc * 32, hipMemcpyDeviceToHost, s.stream));
        rc = sync_unlocked(ctx, lk, s.stream, what);
        if (rc) return rc;
        if (herr != 0xffffffffu) {
            ctx->last_error = std::string(what) + ": polynomial " + std::to_string(b0 + (herr >> lg)) + ": value " +
                              std::to_string(herr & (n - 1)) + " is not below r";
            return KZG_ERR_INVALID_ARG;
        }
    }
    return KZG_OK;
}

// the arguments of the two evaluation-form entry points; *lg receives log2 n
static int bary_check(kzg_ctx* ctx, const char* what, const uint64_t* evals, size_t n, size_t batch, size_t stride,
                      const uint64_t* zs, uint32_t* lg) {
    auto invalid = [&](const std::string& why) {
        ctx->last_error = std::string(what) + ": " + why;
        return KZG_ERR_INVALID_ARG;
    };
    if (!ntt_log(n, lg)) return invalid("n is not a power of two up to 2^KZG_NTT_MAX_LOG");
    if (batch && (!evals || !zs)) return invalid("a required pointer is NULL");
    if (batch > 1 && stride < n) return invalid("stride < n");
    return KZG_OK;
}
// ... and their points and values below r (after a multi-device context has forwarded: its device's context checks them)
static int bary_check_values(kzg_ctx* ctx, const char* what, const uint64_t* evals, size_t n, size_t batch, size_t stride,
                             const uint64_t* zs) {
    auto invalid = [&](const std::string& why) {
        ctx->last_error = std::string(what) + ": " + why;
        return KZG_ERR_INVALID_ARG;
    };
    for (size_t b = 0; b < batch; b++) {
        hf::Fr v;
        std::memcpy(v.l, zs + 4 * b, 32);
        if (hf::fr_geq(v, hf::kFrMod)) return invalid("polynomial " + std::to_string(b) + ": the point is not below r");
        for (size_t i = 0; i < n; i++) {
            std::memcpy(v.l, evals + 4 * (b * stride + i), 32);
            if (hf::fr_geq(v, hf::kFrMod))
                return invalid("polynomial " + std::to_string(b) + ": value " + std::to_string(i) + " is not below r");
        }
    }
    return KZG_OK;
}

int kzg_evaluate_evaluations_batch(kzg_ctx* ctx, const uint64_t* evals_fr_mont, size_t n, size_t batch, size_t stride,
                                   const uint64_t* zs, uint64_t* out_ys) {
    if (!ctx) return KZG_ERR_INVALID_ARG;
    uint32_t lg = 0;
    const int rc = bary_check(ctx, "evaluate evaluations", evals_fr_mont, n, batch, stride, zs, &lg);
    if (rc) return rc;
    if (batch && !out_ys) {
        ctx->last_error = "evaluate evaluations: a required pointer is NULL";
        return KZG_ERR_INVALID_ARG;
    }
    if (!batch) return KZG_OK;
    if (ctx->multi) {
        kzg_ctx* kid = multi_kid(ctx->multi, 0);
        return forwarded(ctx, kid, kzg_evaluate_evaluations_batch(kid, evals_fr_mont, n, batch, stride, zs, out_ys));
    }
    const int rcv = bary_check_values(ctx, "evaluate evaluations", evals_fr_mont, n, batch, stride, zs);
    if (rcv) return rcv;
    return bary_host(ctx, evals_fr_mont, lg, batch, stride, zs, nullptr, out_ys);
}

// Record t: commitment commitment_idx[t] (t itself when commitment_idx is null) opens to y_t at z_t with proof t.  ys on the
// host, or d_ys: the k values in the kVcCells workspace already (fk20_mu held by the caller).  weights as verify_cells_impl.
static int verify_openings_impl(kzg_ctx* ctx, const uint64_t* commitments_p1, size_t num_commitments, const uint32_t* commitment_idx,
                                const uint64_t* zs, const uint64_t* ys, const uint32_t* d_ys, const uint64_t* proofs_p1, size_t k,
                                const void* setup_g2, size_t g2_stride_bytes, const uint64_t* weights, bool want_weights,
                                uint64_t* out_lhs, uint64_t* out_rhs, int* valid, const VcWire* wire = nullptr) {
    if (!ctx) return KZG_ERR_INVALID_ARG;
    const char* what = "verify openings";
    auto invalid = [&](const std::string& why) {
        ctx->last_error = std::string(what) + ": " + why;
        return KZG_ERR_INVALID_ARG;
    };
    if (k > KZG_VERIFY_MAX_OPENINGS) return invalid("more than KZG_VERIFY_MAX_OPENINGS records");
    if (num_commitments > KZG_VERIFY_MAX_OPENINGS) return invalid("more than KZG_VERIFY_MAX_OPENINGS commitments");
    // wire (section 4.12): the commitments and proofs are its byte strings, and so are the points and the claimed values
    // unless they come decoded (zs) or on the device (d_ys), as from kzg_verify_blobs_batch_bytes
    const void* in_commitments = wire ? (const void*)wire->commitments48 : commitments_p1;
    const void* in_proofs = wire ? (const void*)wire->proofs48 : proofs_p1;
    const void* in_zs = wire && wire->zs_be ? (const void*)wire->zs_be : zs;
    const void* in_ys = wire ? (const void*)wire->values_be : ys;
    if (!valid || (want_weights && (!out_lhs || !out_rhs)) || (num_commitments && !in_commitments) ||
        (k && ((!commitment_idx && !d_ys) || !in_zs || (!in_ys && !d_ys) || !in_proofs || !setup_g2 || (want_weights && !weights))))
        return invalid("a required pointer is NULL");
    if (!k) {
        if (want_weights) {
            const hf::P1 inf = hf::p1_inf();
            write_p1(out_lhs, inf);
            write_p1(out_rhs, inf);
        }
        *valid = 1;
        return KZG_OK;
    }
    if (ctx->multi) {  // before the O(k) checks, which the device's context makes (kzg_verify_evaluations_batch forwards itself)
        int rc = KZG_OK;
        kzg_ctx* kid = cells_kid(ctx, &rc);
        return kid ? forwarded(ctx, kid, verify_openings_impl(kid, commitments_p1, num_commitments, commitment_idx, zs, ys, d_ys,
                                                              proofs_p1, k, setup_g2, g2_stride_bytes, weights, want_weights,
                                                              out_lhs, out_rhs, valid, wire))
                   : rc;
    }
    if (commitment_idx)
        for (size_t t = 0; t < k; t++)
            if (commitment_idx[t] >= num_commitments)
                return invalid("record " + std::to_string(t) + ": commitment index " + std::to_string(commitment_idx[t]) +
                               " is not below num_commitments");
    std::vector<uint64_t> own_zs;
    if (wire && wire->zs_be) {  // the host groups the records by point and splits the points: it decodes them
        own_zs.resize(4 * k);
        for (size_t t = 0; t < k; t++)
            if (!wire_fr_host(wire->zs_be + 32 * t, own_zs.data() + 4 * t))
                return invalid("record " + std::to_string(t) + ": the point z is not below r");
        zs = own_zs.data();
    }
    if (ys)  // (with d_ys the caller has checked the points and the device has made the values)
        for (size_t t = 0; t < k; t++) {
            hf::Fr v;
            std::memcpy(v.l, zs + 4 * t, 32);
            if (hf::fr_geq(v, hf::kFrMod)) return invalid("record " + std::to_string(t) + ": the point is not below r");
            std::memcpy(v.l, ys + 4 * t, 32);
            if (hf::fr_geq(v, hf::kFrMod)) return invalid("record " + std::to_string(t) + ": the value is not below r");
        }
    hf::G2Affine g2[2];
    {
        const int rci = vc_check_inputs(ctx, what, want_weights ? weights : nullptr, proofs_p1, k, commitments_p1, num_commitments,
                                        setup_g2, g2_stride_bytes, 1, "1", g2, wire != nullptr);
        if (rci) return rci;
    }
    CellsShape sh;
    cells_shape(0, 0, 0, &sh);  // l = 1
    VcBatch vb;
    vb.sh = &sh;
    vb.k = k;
    vb.B = num_commitments;
    vb.commitments = commitments_p1;
    vb.cells = ys;
    vb.d_values = d_ys;
    vb.fk20_held = d_ys != nullptr;
    vb.proofs = proofs_p1;
    vb.what = what;
    if (wire) {
        vb.wire_commitments = wire->commitments48;
        vb.wire_proofs = wire->proofs48;
        vb.wire_values = d_ys ? nullptr : wire->values_be;
    }
    std::vector<hf::Fr> rho;
    {
        const int rcw = vc_weights(ctx, what, want_weights ? weights : nullptr, k, &rho, &vb.glv);
        if (rcw) return rcw;
    }
    // records sorted by point (the 32-byte images, ties by record), the distinct points and their counts
    vb.order.resize(k);
    for (size_t t = 0; t < k; t++) vb.order[t] = (uint32_t)t;
    std::sort(vb.order.begin(), vb.order.end(), [&](uint32_t a, uint32_t b) {
        const int c = std::memcmp(zs + 4 * a, zs + 4 * b, 32);
        return c ? c < 0 : a < b;
    });
    for (size_t t = 0; t < k; t++) {
        const uint64_t* z = zs + 4 * vb.order[t];
        if (t && !std::memcmp(z, zs + 4 * vb.order[t - 1], 32)) {
            vb.lens.back()++;
            continue;
        }
        hf::Fr v;
        std::memcpy(v.l, z, 32);
        vb.ids.push_back((uint32_t)vb.ids.size());
        vb.lens.push_back(1);
        vb.points.push_back(glv_split(v));
    }
    vb.rho30.resize(k);
    for (size_t t = 0; t < k; t++) vb.rho30[t] = fr30_arg_from_mont256(rho[vb.order[t]]);
    const hf::Fr zero = {{0, 0, 0, 0}};
    vb.U.assign(num_commitments, zero);
    for (size_t t = 0; t < k; t++) {
        const size_t b = commitment_idx ? commitment_idx[t] : t;
        vb.U[b] = hf::fr_add(vb.U[b], rho[t]);
    }
    uint64_t lhs[18], rhs[18];
    const int rc = vc_device(ctx, vb, lhs, rhs);
    if (rc) return rc;
    if (want_weights) {
        std::memcpy(out_lhs, lhs, sizeof lhs);
        std::memcpy(out_rhs, rhs, sizeof rhs);
    }
    *valid = vc_pair(lhs, rhs, g2[1], g2[0]);  // e(LHS, [s]G2) == e(RHS, G2)
    return KZG_OK;
}

int kzg_verify_openings_batch(kzg_ctx* ctx, const uint64_t* commitments_p1, size_t num_commitments, const uint32_t* commitment_idx,
                              const uint64_t* zs, const uint64_t* ys, const uint64_t* proofs_p1, size_t k, const void* setup_g2,
                              size_t g2_stride_bytes, int* valid) {
    if (ctx && k && (!commitment_idx || !ys)) {
        ctx->last_error = "verify openings: a required pointer is NULL";
        return KZG_ERR_INVALID_ARG;
    }
    return verify_openings_impl(ctx, commitments_p1, num_commitments, commitment_idx, zs, ys, nullptr, proofs_p1, k, setup_g2,
                                g2_stride_bytes, nullptr, false, nullptr, nullptr, valid);
}

int kzg_verify_openings_lincomb(kzg_ctx* ctx, const uint64_t* commitments_p1, size_t num_commitments, const uint32_t* commitment_idx,
                                const uint64_t* zs, const uint64_t* ys, const uint64_t* proofs_p1, size_t k, const void* setup_g2,
                                size_t g2_stride_bytes, const uint64_t* weights, uint64_t out_lhs_p1[18], uint64_t out_rhs_p1[18],
                                int* valid) {
    if (ctx && k && (!commitment_idx || !ys)) {
        ctx->last_error = "verify openings: a required pointer is NULL";
        return KZG_ERR_INVALID_ARG;
    }
    return verify_openings_impl(ctx, commitments_p1, num_commitments, commitment_idx, zs, ys, nullptr, proofs_p1, k, setup_g2,
                                g2_stride_bytes, weights, true, out_lhs_p1, out_rhs_p1, valid);
}

namespace {
// kzg_verify_blobs_batch_bytes's inputs (section 4.12); evals_fr_mont, commitments_p1, zs, proofs_p1 and out_ys are null then
struct BlobWire {
    const uint8_t* blobs_be;
    unsigned order;
    const uint8_t* commitments48;
    const uint8_t* zs_be;
    const uint8_t* proofs48;
    uint8_t* out_ys_be;
};
}  // namespace

static int verify_evaluations_impl(kzg_ctx* ctx, const uint64_t* evals_fr_mont, size_t n, size_t batch, size_t stride,
                                   const uint64_t* commitments_p1, const uint64_t* zs, const uint64_t* proofs_p1, const void* setup_g2,
                                   size_t g2_stride_bytes, uint64_t* out_ys, int* valid, const BlobWire* wire) {
    if (!ctx) return KZG_ERR_INVALID_ARG;
    const char* what = wire ? "verify blobs" : "verify evaluations";
    auto invalid = [&](const std::string& why) {
        ctx->last_error = std::string(what) + ": " + why;
        return KZG_ERR_INVALID_ARG;
    };
    uint32_t lg = 0;
    int rc = bary_check(ctx, what, wire ? (const uint64_t*)wire->blobs_be : evals_fr_mont, n, batch, stride,
                        wire ? (const uint64_t*)wire->zs_be : zs, &lg);
    if (rc) return rc;
    if (wire && wire->order != KZG_ORDER_NATURAL && wire->order != KZG_ORDER_BIT_REVERSED)
        return invalid("order is neither KZG_ORDER_NATURAL nor KZG_ORDER_BIT_REVERSED");
    if (batch > KZG_VERIFY_MAX_OPENINGS) return invalid("more than KZG_VERIFY_MAX_OPENINGS polynomials");
    if (!valid || (batch && (!(wire ? (const void*)wire->commitments48 : commitments_p1) ||
                             !(wire ? (const void*)wire->proofs48 : proofs_p1) || !setup_g2)))
        return invalid("a required pointer is NULL");
    if (!batch) {
        *valid = 1;
        return KZG_OK;
    }
    if (ctx->multi) {
        kzg_ctx* kid = cells_kid(ctx, &rc);
        return kid ? forwarded(ctx, kid, verify_evaluations_impl(kid, evals_fr_mont, n, batch, stride, commitments_p1, zs, proofs_p1,
                                                                 setup_g2, g2_stride_bytes, out_ys, valid, wire))
                   : rc;
    }
    std::vector<uint64_t> own_zs, own_ys;
    if (wire) {  // the points on the host (the verifier groups and splits them); the values on the device, chunk by chunk
        own_zs.resize(4 * batch);
        for (size_t b = 0; b < batch; b++)
            if (!wire_fr_host(wire->zs_be + 32 * b, own_zs.data() + 4 * b))
                return invalid("polynomial " + std::to_string(b) + ": the point z is not below r");
        zs = own_zs.data();
        if (wire->out_ys_be) {
            own_ys.resize(4 * batch);
            out_ys = own_ys.data();
        }
    } else {
        rc = bary_check_values(ctx, what, evals_fr_mont, n, batch, stride, zs);
        if (rc) return rc;
    }
    // the values go from the evaluation straight into the verifier's value buffer: fk20_mu guards that workspace for both
    std::lock_guard<std::mutex> lkf(ctx->fk20_mu);
    void* d_ys = nullptr;
    {
        std::unique_lock<std::mutex> lk(ctx->mu);
        if (!ctx->n || !ctx->slots_ready) {
            ctx->last_error = std::string(what) + ": the SRS is empty";
            return KZG_ERR_NO_SRS;
        }
        HIP_TRY(ctx, hipSetDevice(ctx->device));
        rc = ctx->vc_ws.get(ctx, kVcCells, batch * 32, &d_ys);
        if (rc) return rc;
    }
    rc = bary_host(ctx, evals_fr_mont, lg, batch, stride, zs, (uint32_t*)d_ys, out_ys, wire ? wire->blobs_be : nullptr,
                   wire && wire->order == KZG_ORDER_BIT_REVERSED, what);
    if (rc) return rc;
    if (wire && wire->out_ys_be)
        for (size_t b = 0; b < batch; b++) wire_fr_to_be(own_ys.data() + 4 * b, wire->out_ys_be + 32 * b);
    VcWire vw;
    if (wire) {
        vw.commitments48 = wire->commitments48;
        vw.proofs48 = wire->proofs48;
    }
    return verify_openings_impl(ctx, commitments_p1, batch, nullptr, zs, nullptr, (const uint32_t*)d_ys, proofs_p1, batch, setup_g2,
                                g2_stride_bytes, nullptr, false, nullptr, nullptr, valid, wire ? &vw : nullptr);
}

int kzg_verify_evaluations_batch(kzg_ctx* ctx, const uint64_t* evals_fr_mont, size_t n, size_t batch, size_t stride,
                                 const uint64_t* commitments_p1, const uint64_t* zs, const uint64_t* proofs_p1, const void* setup_g2,
                                 size_t g2_stride_bytes, uint64_t* out_ys, int* valid) {
    return verify_evaluations_impl(ctx, evals_fr_mont, n, batch, stride, commitments_p1, zs, proofs_p1, setup_g2, g2_stride_bytes,
                                   out_ys, valid, nullptr);
}

// ---- the verifiers on inputs as they travel (wire_kernels.hip) -------------------------------------------

int kzg_verify_cells_batch_bytes(kzg_ctx* ctx, const uint8_t* commitments48, size_t num_commitments, const uint32_t* commitment_idx,
                                 const uint32_t* cell_ids, const uint8_t* cells_be, const uint8_t* proofs48, size_t k,
                                 unsigned log_domain, unsigned log_cell, unsigned order, const void* setup_g2, size_t g2_stride_bytes,
                                 int* valid) {
    VcWire w;
    w.commitments48 = commitments48;
    w.proofs48 = proofs48;
    w.values_be = cells_be;
    w.order = order;
    return verify_cells_impl(ctx, nullptr, num_commitments, commitment_idx, cell_ids, nullptr, nullptr, k, log_domain, log_cell,
                             setup_g2, g2_stride_bytes, nullptr, false, nullptr, nullptr, valid, &w);
}

int kzg_verify_cells_lincomb_bytes(kzg_ctx* ctx, const uint8_t* commitments48, size_t num_commitments, const uint32_t* commitment_idx,
                                   const uint32_t* cell_ids, const uint8_t* cells_be, const uint8_t* proofs48, size_t k,
                                   unsigned log_domain, unsigned log_cell, unsigned order, const void* setup_g2,
                                   size_t g2_stride_bytes, const uint64_t* weights, uint64_t out_lhs_p1[18], uint64_t out_rhs_p1[18],
                                   int* valid) {
    VcWire w;
    w.commitments48 = commitments48;
    w.proofs48 = proofs48;
    w.values_be = cells_be;
    w.order = order;
    return verify_cells_impl(ctx, nullptr, num_commitments, commitment_idx, cell_ids, nullptr, nullptr, k, log_domain, log_cell,
                             setup_g2, g2_stride_bytes, weights, true, out_lhs_p1, out_rhs_p1, valid, &w);
}

static int verify_openings_bytes(kzg_ctx* ctx, const uint8_t* commitments48, size_t num_commitments, const uint32_t* commitment_idx,
                                 const uint8_t* zs_be, const uint8_t* ys_be, const uint8_t* proofs48, size_t k, const void* setup_g2,
                                 size_t g2_stride_bytes, const uint64_t* weights, bool want_weights, uint64_t* out_lhs,
                                 uint64_t* out_rhs, int* valid) {
    if (ctx && k && (!commitment_idx || !ys_be)) {
        ctx->last_error = "verify openings: a required pointer is NULL";
        return KZG_ERR_INVALID_ARG;
    }
    VcWire w;
    w.commitments48 = commitments48;
    w.proofs48 = proofs48;
    w.values_be = ys_be;
    w.zs_be = zs_be;
    return verify_openings_impl(ctx, nullptr, num_commitments, commitment_idx, nullptr, nullptr, nullptr, nullptr, k, setup_g2,
                                g2_stride_bytes, weights, want_weights, out_lhs, out_rhs, valid, &w);
}

int kzg_verify_openings_batch_bytes(kzg_ctx* ctx, const uint8_t* commitments48, size_t num_commitments, const uint32_t* commitment_idx,
                                    const uint8_t* zs_be, const uint8_t* ys_be, const uint8_t* proofs48, size_t k,
                                    const void* setup_g2, size_t g2_stride_bytes, int* valid) {
    return verify_openings_bytes(ctx, commitments48, num_commitments, commitment_idx, zs_be, ys_be, proofs48, k, setup_g2,
                                 g2_stride_bytes, nullptr, false, nullptr, nullptr, valid);
}

int kzg_verify_openings_lincomb_bytes(kzg_ctx* ctx, const uint8_t* commitments48, size_t num_commitments,
                                      const uint32_t* commitment_idx, const uint8_t* zs_be, const uint8_t* ys_be,
                                      const uint8_t* proofs48, size_t k, const void* setup_g2, size_t g2_stride_bytes,
                                      const uint64_t* weights, uint64_t out_lhs_p1[18], uint64_t out_rhs_p1[18], int* valid) {
    return verify_openings_bytes(ctx, commitments48, num_commitments, commitment_idx, zs_be, ys_be, proofs48, k, setup_g2,
                                 g2_stride_bytes, weights, true, out_lhs_p1, out_rhs_p1, valid);
}

int kzg_verify_blobs_batch_bytes(kzg_ctx* ctx, const uint8_t* blobs_be, size_t n, size_t batch, size_t stride, unsigned order,
                                 const uint8_t* commitments48, const uint8_t* zs_be, const uint8_t* proofs48, const void* setup_g2,
                                 size_t g2_stride_bytes, uint8_t* out_ys_be, int* valid) {
    const BlobWire w = {blobs_be, order, commitments48, zs_be, proofs48, out_ys_be};
    return verify_evaluations_impl(ctx, nullptr, n, batch, stride, nullptr, nullptr, nullptr, setup_g2, g2_stride_bytes, nullptr,
                                   valid, &w);
}

// the decoders on their own: building blocks and test hooks; they need no SRS
int kzg_g1_uncompress_batch(kzg_ctx* ctx, const uint8_t* in48, size_t n, int check_subgroup, uint64_t* out_p1, size_t* bad_index) {
    if (!ctx) return KZG_ERR_INVALID_ARG;
    if (bad_index) *bad_index = (size_t)-1;
    if (n > kMaxCoefficients - 1 || (n && (!in48 || !out_p1))) {
        ctx->last_error = "g1 uncompress: a required pointer is NULL or n does not fit 32 bits";
        return KZG_ERR_INVALID_ARG;
    }
    if (!n) return KZG_OK;
    if (ctx->multi) {
        kzg_ctx* kid = multi_kid(ctx->multi, 0);
        return forwarded(ctx, kid, kzg_g1_uncompress_batch(kid, in48, n, check_subgroup, out_p1, bad_index));
    }
    std::lock_guard<std::mutex> lkf(ctx->fk20_mu);
    std::unique_lock<std::mutex> lk(ctx->mu);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const int slot = reserve_slot(ctx, lk, true);
    if (slot < 0) return KZG_ERR_BUSY;
    SlotLease lease{ctx, slot};
    Slot& s = ctx->slots[slot];
    int rc = ensure_slot_basics(ctx, s);
    void *p1 = nullptr, *aff = nullptr, *coef = nullptr, *dglv = nullptr, *g1 = nullptr;
    if (rc == KZG_OK) rc = ctx->vc_ws.get(ctx, kVcP1, n * 144, &p1);
    if (rc == KZG_OK) rc = ctx->vc_ws.get(ctx, kVcAff, n * kAffineBytes, &aff);
    if (rc == KZG_OK) rc = ctx->vc_ws.get(ctx, kVcCoefA, kVcErrWords * 4, &coef);
    if (rc == KZG_OK && check_subgroup) rc = ctx->vc_ws.get(ctx, kVcGlv, n * sizeof(Glv), &dglv);
    if (rc == KZG_OK && check_subgroup) rc = ctx->vc_ws.get(ctx, kVcG1, n * kXyzzBytes, &g1);
    if (rc) return rc;
    const hipStream_t st = s.stream;
    uint32_t* err = (uint32_t*)coef;
    HIP_TRY(ctx, hipMemsetAsync(err, 0xff, kVcErrWords * 4, st));
    HIP_TRY(ctx, hipMemcpyAsync(p1, in48, n * 48, hipMemcpyHostToDevice, st));
    launch_wire_g1(st, p1, nullptr, (uint32_t)n, aff, (uint32_t)kAffineBytes, err + kVcErrWireProof);
    if (check_subgroup) {  // the ladder's membership test with a weight of zero: [0] P costs nothing
        HIP_TRY(ctx, hipMemsetAsync(dglv, 0, n * sizeof(Glv), st));
        launch_vc_ladder(st, aff, nullptr, (const Glv*)dglv, (uint32_t)n, (uint32_t)n, (uint32_t)n, g1, g1, err);
    }
    launch_affine_to_p1(st, aff, (uint32_t)n, p1);
    HIP_TRY(ctx, hipGetLastError());
    uint32_t herr[kVcErrWords];
    HIP_TRY(ctx, hipMemcpyAsync(herr, err, sizeof herr, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipMemcpyAsync(out_p1, p1, n * 144, hipMemcpyDeviceToHost, st));
    rc = sync_unlocked(ctx, lk, st, "g1 uncompress");
    if (rc) return rc;
    const uint32_t enc = herr[kVcErrWireProof], grp = std::min(herr[kVcErrCurve], herr[kVcErrG1]);
    if (enc != 0xffffffffu || grp != 0xffffffffu) {
        const uint32_t bad = std::min(enc, grp);
        if (bad_index) *bad_index = bad;
        ctx->last_error = "g1 uncompress: point " + std::to_string(bad) + (bad == enc ? " is not a valid compressed point" : " is not in G1");
        return KZG_ERR_INVALID_ARG;
    }
    return KZG_OK;
}

// ---- a Lagrange basis given as compressed points ---------------------------------------------------
// n x 48 bytes -> n affine records in natural order at aff (device), decoded on the device with the subgroup check always on;
// bit-reversed input: record i is point brp(i) of the input.  wire: n x 48 bytes, src: n words (bit-reversed order only), err:
// kVcErrWords words, dglv: n Glv records, g1: n XYZZ records.  Enqueues only; *herr receives the error words once st is waited for.
static int lagrange_enqueue_decode(kzg_ctx* ctx, hipStream_t st, const uint8_t* in48, size_t n, uint32_t lg, bool bit_reversed, void* wire,
                                   uint32_t* src, std::vector<uint32_t>& h_src, uint32_t* err, void* dglv, void* g1, void* aff,
                                   uint32_t herr[kVcErrWords]) {
    HIP_TRY(ctx, hipMemsetAsync(err, 0xff, kVcErrWords * 4, st));
    HIP_TRY(ctx, hipMemcpyAsync(wire, in48, n * 48, hipMemcpyHostToDevice, st));
    if (bit_reversed) {
        h_src.resize(n);
        for (size_t i = 0; i < n; i++) h_src[i] = lagrange_brp((uint32_t)i, lg);
        HIP_TRY(ctx, hipMemcpyAsync(src, h_src.data(), n * 4, hipMemcpyHostToDevice, st));
    }
    launch_wire_g1(st, wire, bit_reversed ? src : nullptr, (uint32_t)n, aff, (uint32_t)kAffineBytes, err + kVcErrWireProof);
    HIP_TRY(ctx, hipMemsetAsync(dglv, 0, n * sizeof(Glv), st));  // the ladder's membership test with a weight of zero
    launch_vc_ladder(st, aff, nullptr, (const Glv*)dglv, (uint32_t)n, (uint32_t)n, (uint32_t)n, g1, g1, err);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipMemcpyAsync(herr, err, kVcErrWords * 4, hipMemcpyDeviceToHost, st));
    return KZG_OK;
}
// the verdict on the decoded points: the input index of a point that does not decode or lies outside G1
static int lagrange_decode_verdict(kzg_ctx* ctx, const uint32_t herr[kVcErrWords], uint32_t lg, bool bit_reversed, size_t* bad_index) {
    const uint32_t enc = herr[kVcErrWireProof];  // an input index already
    uint32_t grp = std::min(herr[kVcErrCurve], herr[kVcErrG1]);  // a record index: natural order
    if (grp != 0xffffffffu && bit_reversed) grp = lagrange_brp(grp, lg);
    if (enc == 0xffffffffu && grp == 0xffffffffu) return KZG_OK;
    const uint32_t bad = std::min(enc, grp);
    if (bad_index) *bad_index = bad;
    ctx->last_error = "lagrange basis: point " + std::to_string(bad) + (bad == enc ? " is not a valid compressed point" : " is not in G1");
    return KZG_ERR_INVALID_ARG;
}

int kzg_lagrange_load_compressed(kzg_ctx* ctx, const uint8_t* in48, size_t n, unsigned order, int check, size_t* bad_index,
                                 int* consistent) {
    uint32_t lg = 0;
    if (bad_index) *bad_index = (size_t)-1;
    if (consistent) *consistent = 0;
    if (!ctx || !in48 || !ntt_log(n, &lg) || order > KZG_ORDER_BIT_REVERSED || (check && !consistent)) return KZG_ERR_INVALID_ARG;
    if (ctx->multi) {
        int rc = KZG_OK;
        kzg_ctx* kid = lagrange_kid(ctx, &rc);
        return kid ? forwarded(ctx, kid, kzg_lagrange_load_compressed(kid, in48, n, order, check, bad_index, consistent)) : rc;
    }
    const bool bit_reversed = order == KZG_ORDER_BIT_REVERSED;
    std::lock_guard<std::mutex> lkf(ctx->fk20_mu);
    std::unique_lock<std::mutex> lk(ctx->mu);
    if (!ctx->n || !ctx->slots_ready) return KZG_ERR_NO_SRS;
    if (n > ctx->n) return KZG_ERR_DEGREE_TOO_HIGH;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    DevBuf tab;
    const uint64_t gen = ctx->srs_gen;
    {
        const int slot = reserve_slot(ctx, lk, true);  // (keeps an SRS replacement out while ctx->mu is released below)
        if (slot < 0) return KZG_ERR_BUSY;
        SlotLease lease{ctx, slot};
        Slot& s = ctx->slots[slot];
        const hipStream_t st = s.stream;
        DevBuf wire, src, err, dglv, g1, prefix;
        int rc = tab.reserve(ctx, (size_t)ctx->cfg.W * n * kAffineBytes);
        if (rc == KZG_OK) rc = wire.reserve(ctx, n * 48);
        if (rc == KZG_OK) rc = src.reserve(ctx, n * 4);
        if (rc == KZG_OK) rc = err.reserve(ctx, kVcErrWords * 4);
        if (rc == KZG_OK) rc = dglv.reserve(ctx, n * sizeof(Glv));
        if (rc == KZG_OK) rc = g1.reserve(ctx, n * kXyzzBytes);
        if (rc == KZG_OK) rc = prefix.reserve(ctx, n * 64);
        if (rc) return rc;
        std::vector<uint32_t> h_src;
        uint32_t herr[kVcErrWords];
        rc = lagrange_enqueue_decode(ctx, st, in48, n, lg, bit_reversed, wire.p, src.dev(), h_src, err.dev(), dglv.p, g1.p, tab.p, herr);
        if (rc == KZG_OK) rc = sync_unlocked(ctx, lk, st, "lagrange basis");
        if (rc == KZG_OK) rc = lagrange_decode_verdict(ctx, herr, lg, bit_reversed, bad_index);
        if (rc) return rc;
        lagrange_enqueue_levels(ctx, st, tab.p, n, g1.p, prefix.p);
        HIP_TRY(ctx, hipGetLastError());
        rc = sync_unlocked(ctx, lk, st, "lagrange basis");
        if (rc) return rc;
        if (check) {
            // sum_i rho_i L_i against sum_j (inverse NTT of rho)_j SRS[j] for n weights of 128 random bits: two MSMs through
            // the slot, the first over the given table.  The weights are read as blst_fr images on both sides (the transform is
            // linear, so the factor 2^-256 they then carry is common to both).
            std::vector<uint64_t> rho(4 * n, 0);
            std::vector<uint64_t> r128(2 * n);
            if (!vc_random(r128.data(), r128.size() * 8)) {
                ctx->last_error = "lagrange basis: getrandom failed";
                return KZG_ERR_HIP;
            }
            for (size_t i = 0; i < n; i++) {
                rho[4 * i] = r128[2 * i];
                rho[4 * i + 1] = r128[2 * i + 1];
            }
            rc = lagrange_slot_ready(ctx, s, n, lg);
            if (rc) return rc;
            uint32_t* d_rho = ntt_slot_input(s, lg);
            rc = copy_unlocked(ctx, lk, st, d_rho, rho.data(), n * 32, hipMemcpyHostToDevice, "hipMemcpyAsync (weights)");
            if (rc == KZG_OK) rc = sync_unlocked(ctx, lk, st, "lagrange basis");  // rho is pageable host memory
            if (rc) return rc;
            uint64_t sides[2][18];
            const MsmBasis given{tab.p, (uint32_t)n};
            rc = submit_commit_locked(ctx, slot, d_rho, 1, n, true, true, &given);
            if (rc) return rc;
            await_unlocked(lk, s);
            rc = wait_locked(ctx, slot, sides[0]);
            if (rc) return rc;
            s.kind = SLOT_RESERVED;  // (wait_locked marked the slot idle; it stays this call's)
            rc = ntt_into_stage(ctx, s, d_rho, lg, true);
            if (rc == KZG_OK) rc = submit_commit_locked(ctx, slot, s.stage.dev(), 1, n, true, true);
            if (rc) return rc;
            await_unlocked(lk, s);
            rc = wait_locked(ctx, slot, sides[1]);
            if (rc) return rc;
            s.kind = SLOT_RESERVED;
            *consistent = std::memcmp(sides[0], sides[1], sizeof sides[0]) == 0 ? 1 : 0;
            if (!*consistent) return KZG_OK;  // not adopted
        }
    }
    return lagrange_adopt(ctx, lk, tab, n, gen);
}

int kzg_srs_load_lagrange_compressed(kzg_ctx* ctx, const uint8_t* in48, size_t n, unsigned order, size_t* bad_index) {
    uint32_t lg = 0;
    if (bad_index) *bad_index = (size_t)-1;
    if (!ctx || !in48 || !ntt_log(n, &lg) || order > KZG_ORDER_BIT_REVERSED) return KZG_ERR_INVALID_ARG;
    if (ctx->multi) {
        ctx->last_error = "kzg_srs_load_lagrange_compressed takes a single-device context: load the monomial form it returns "
                          "(kzg_srs_read_g1) into a multi-device one";
        return KZG_ERR_INVALID_ARG;
    }
    const bool bit_reversed = order == KZG_ORDER_BIT_REVERSED;
    std::lock_guard<std::mutex> lkf(ctx->fk20_mu);
    std::unique_lock<std::mutex> lk(ctx->mu);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    TmpStream st;
    HIP_TRY(ctx, hipStreamCreateWithFlags(&st.s, hipStreamNonBlocking));
    int rc = ensure_glv(ctx, lk, lg, st.s);  // (releases ctx->mu while it waits: before the quiesce)
    if (rc) return rc;
    quiesce(ctx, lk);
    // decode first: a malformed input leaves the context as it was
    DevBuf aff, wire, src, err, dglv, x1, x2, x3, prefix;
    rc = aff.reserve(ctx, n * kAffineBytes);
    if (rc == KZG_OK) rc = wire.reserve(ctx, n * 48);
    if (rc == KZG_OK) rc = src.reserve(ctx, n * 4);
    if (rc == KZG_OK) rc = err.reserve(ctx, kVcErrWords * 4);
    if (rc == KZG_OK) rc = dglv.reserve(ctx, n * sizeof(Glv));
    if (rc == KZG_OK) rc = x1.reserve(ctx, n * kXyzzBytes);
    if (rc == KZG_OK) rc = x2.reserve(ctx, n * kXyzzBytes);
    if (rc == KZG_OK) rc = x3.reserve(ctx, n * kXyzzBytes);
    if (rc == KZG_OK) rc = prefix.reserve(ctx, n * 64);
    if (rc) return rc;
    std::vector<uint32_t> h_src;
    uint32_t herr[kVcErrWords];
    rc = lagrange_enqueue_decode(ctx, st.s, in48, n, lg, bit_reversed, wire.p, src.dev(), h_src, err.dev(), dglv.p, x1.p, aff.p, herr);
    if (rc) return rc;
    HIP_TRY(ctx, hipStreamSynchronize(st.s));
    rc = lagrange_decode_verdict(ctx, herr, lg, bit_reversed, bad_index);
    if (rc) return rc;
    // SRS[j] = sum_i w^(ij) L_i: the forward G1 DFT into level 0, then the normal ingest path
    rc = srs_prepare(ctx, n);
    if (rc) return rc;
    launch_affine_to_xyzz(st.s, aff.p, n, x1.p);
    const void* res = launch_g1_dft(st.s, x1.p, x2.p, x3.p, lg, 1, (const Glv*)ctx->glv.p, ctx->glv_log, false);
    launch_xyzz_to_affine(st.s, res, (uint32_t)n, ctx->table.p, prefix.p);
    HIP_TRY(ctx, hipGetLastError());
    rc = finish_srs_from_level0(ctx, st.s, n);
    if (rc) return rc;
    // the decoded points are the Lagrange basis of the new setup
    DevBuf tab;
    rc = tab.reserve(ctx, (size_t)ctx->cfg.W * n * kAffineBytes);
    if (rc) return rc;
    HIP_TRY(ctx, hipMemcpyAsync(tab.p, aff.p, n * kAffineBytes, hipMemcpyDeviceToDevice, st.s));
    lagrange_enqueue_levels(ctx, st.s, tab.p, n, x1.p, prefix.p);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipStreamSynchronize(st.s));
    std::swap(ctx->lag_table.p, tab.p);
    std::swap(ctx->lag_table.cap, tab.cap);
    ctx->lag_n = n;
    return KZG_OK;
}

int kzg_fr_from_bytes_batch(kzg_ctx* ctx, const uint8_t* in32_be, size_t n, uint64_t* out_fr_mont, size_t* bad_index) {
    if (!ctx) return KZG_ERR_INVALID_ARG;
    if (bad_index) *bad_index = (size_t)-1;
    if (n > kMaxCoefficients - 1 || (n && (!in32_be || !out_fr_mont))) {
        ctx->last_error = "fr from bytes: a required pointer is NULL or n does not fit 32 bits";
        return KZG_ERR_INVALID_ARG;
    }
    if (!n) return KZG_OK;
    if (ctx->multi) {
        kzg_ctx* kid = multi_kid(ctx->multi, 0);
        return forwarded(ctx, kid, kzg_fr_from_bytes_batch(kid, in32_be, n, out_fr_mont, bad_index));
    }
    std::lock_guard<std::mutex> lkf(ctx->fk20_mu);
    std::unique_lock<std::mutex> lk(ctx->mu);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const int slot = reserve_slot(ctx, lk, true);
    if (slot < 0) return KZG_ERR_BUSY;
    SlotLease lease{ctx, slot};
    Slot& s = ctx->slots[slot];
    int rc = ensure_slot_basics(ctx, s);
    void *wire = nullptr, *vals = nullptr, *coef = nullptr;
    if (rc == KZG_OK) rc = ctx->vc_ws.get(ctx, kVcWire, n * 32, &wire);
    if (rc == KZG_OK) rc = ctx->vc_ws.get(ctx, kVcCells, n * 32, &vals);
    if (rc == KZG_OK) rc = ctx->vc_ws.get(ctx, kVcCoefA, kVcErrWords * 4, &coef);
    if (rc) return rc;
    const hipStream_t st = s.stream;
    uint32_t* err = (uint32_t*)coef;
    HIP_TRY(ctx, hipMemsetAsync(err, 0xff, kVcErrWords * 4, st));
    HIP_TRY(ctx, hipMemcpyAsync(wire, in32_be, n * 32, hipMemcpyHostToDevice, st));
    launch_wire_fr(st, wire, (uint32_t)n, 0, false, vals, err + kVcErrWireValue);
    HIP_TRY(ctx, hipGetLastError());
    uint32_t herr = 0;
    HIP_TRY(ctx, hipMemcpyAsync(&herr, err + kVcErrWireValue, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipMemcpyAsync(out_fr_mont, vals, n * 32, hipMemcpyDeviceToHost, st));
    rc = sync_unlocked(ctx, lk, st, "fr from bytes");
    if (rc) return rc;
    if (herr != 0xffffffffu) {
        if (bad_index) *bad_index = herr;
        ctx->last_error = "fr from bytes: value " + std::to_string(herr) + " is not below r";
        return KZG_ERR_INVALID_ARG;
    }
    return KZG_OK;
}

// ---- the producing side on blobs as they travel (blob_kernels.hip) ---------------------------------------
// Blob bytes -> values (k_wire_fr) -> coefficients (one batched inverse DFT; k_poly_trim folds in 1 / n and finds every n') ->
// commitments (the batched MSM over the stream slots, from the resident coefficients), cells (zero-padded to N, one batched
// DFT, one gather, k_enc_fr) and proofs (fk20_proofs from the device source, k_enc_g1).  A call holds fk20_mu, then the
// context's mutex and one slot for its stream, dropping the mutex while it waits for the device, as fk20_host does.
namespace {
enum : int { kBlobWire = 0, kBlobA, kBlobB, kBlobP, kBlobWords, kBlobProofs, kBlobCoef, kBlobP1, kBlobCount };
constexpr uint32_t kBlobErrWords = 2;  // the decoder's error word, the encoder's (never set: the device's values are canonical)
struct Fk20Plan {  // the Toeplitz shape of polynomials of n coefficients and, when the comb tables are not kept, their stream
    uint32_t m = 0, log_L = 0;
    bool ready = false;
    DevBuf stab, stmp, spre;
};
void blob_infinity(uint8_t* out48, size_t count) {
    std::memset(out48, 0, 48 * count);
    for (size_t j = 0; j < count; j++) out48[48 * j] = 0xc0;
}
}  // namespace

// polynomials per pass through the workspaces: fk20_host's rule, with this path's own buffers counted in
static size_t blob_chunk(kzg_ctx* ctx, size_t n, const CellsShape* sh, const Fk20Plan& pl) {
    size_t per_poly = 3 * n * 32;
    if (sh) {
        per_poly += 3 * sh->N * 32 + sh->cells * 48;
        if (pl.m) {
            const size_t L = (size_t)1 << pl.log_L, M = sh->cells, X = L > M ? L : M;
            const size_t ci = ctx->fk20_tab.p ? L : fk20_stream_positions(pl.log_L, sh->log_l);
            per_poly += n * 32 + sh->l * L * 64 + (sh->l > 1 ? sh->l * ci * kXyzzBytes : 0) + 3 * X * kXyzzBytes + M * 336;
        }
    }
    size_t chunk = kFk20WsBudget / per_poly;
    return chunk < 1 ? 1 : (chunk > kFk20MaxBatch ? kFk20MaxBatch : chunk);
}
// (fk20_mu and ctx->mu held, s0 owned) the SRS side of the plan's shape, built on first need
static int blob_fk20_ready(kzg_ctx* ctx, std::unique_lock<std::mutex>& lk, Slot& s0, const CellsShape& sh, Fk20Plan& pl) {
    if (pl.ready) return KZG_OK;
    const uint32_t log_M = sh.log_n - sh.log_l;
    int rc = ensure_glv(ctx, lk, pl.log_L > log_M ? pl.log_L : log_M, s0.stream);
    if (rc == KZG_OK) rc = ensure_fk20_table(ctx, lk, s0.stream, pl.log_L, sh.log_l);
    if (rc) return rc;
    if (!ctx->fk20_tab.p) {
        const size_t sb = (size_t)fk20_stream_positions(pl.log_L, sh.log_l) << sh.log_l;
        HIP_TRY(ctx, hipMalloc(&pl.stab.p, sb * kFk20CombEntries * kAffineBytes));
        HIP_TRY(ctx, hipMalloc(&pl.stmp.p, sb * kFk20CombEntries * kXyzzBytes));
        HIP_TRY(ctx, hipMalloc(&pl.spre.p, sb * kFk20CombEntries * 64));
    }
    pl.ready = true;
    return KZG_OK;
}
// (fk20_mu and ctx->mu held, s0 owned) the proofs of `bc` polynomials whose n coefficients each sit at d_coef, as bc x M x 48
// bytes in the order asked; n_max: the largest n' among them.  Returns with the stream idle.
static int blob_proofs(kzg_ctx* ctx, std::unique_lock<std::mutex>& lk, Slot& s0, const void* d_coef, size_t n, size_t bc,
                       const CellsShape& sh, bool bit_reversed, size_t n_max, Fk20Plan& pl, uint8_t* out48) {
    const size_t M = sh.cells;
    if (n_max <= sh.l) {  // every polynomial is its own interpolant on every cell
        blob_infinity(out48, bc * M);
        return KZG_OK;
    }
    int rc = blob_fk20_ready(ctx, lk, s0, sh, pl);
    if (rc) return rc;
    const uint32_t log_M = sh.log_n - sh.log_l;
    void* enc = nullptr;
    rc = ctx->blob_ws.get(ctx, kBlobProofs, bc * M * 48, &enc);
    if (rc) return rc;
    // all n coefficients, trailing zeros included: one shape for every chunk of the call, the one kzg_fk20_prepare(n) builds
    rc = fk20_proofs(ctx, lk, s0.stream, nullptr, n, bc, n, pl.m, pl.log_L, sh.log_l, log_M, nullptr, pl.stab.p, pl.stmp.p, pl.spre.p,
                     d_coef, true);
    if (rc) return rc;
    launch_enc_g1(s0.stream, ctx->fk20_ws.buf[kWsAff].p, (uint32_t)(bc * M), log_M, bit_reversed, enc);
    HIP_TRY(ctx, hipGetLastError());
    rc = copy_unlocked(ctx, lk, s0.stream, out48, enc, bc * M * 48, hipMemcpyDeviceToHost, "hipMemcpyAsync (blobs)");
    const int r2 = sync_unlocked(ctx, lk, s0.stream, "fk20");
    return rc ? rc : r2;
}

// the commitments of `bc` resident polynomials (n coefficients each at d_coef, none longer than n_c): sub-batches over the
// stream slots, as batch_host spreads them.  submit() enqueues them all (collecting its own oldest when the slots run out),
// finish() collects the rest and compresses.
namespace {
struct BlobCommits {
    kzg_ctx* ctx;
    std::unique_lock<std::mutex>& lk;
    std::deque<BatchInFlight> fifo;
    std::vector<uint64_t> p1;
    int collect_oldest() {
        const BatchInFlight b = fifo.front();
        fifo.pop_front();
        await_unlocked(lk, ctx->slots[b.slot]);
        const int r = wait_batch_locked(ctx, b.slot, p1.data() + 18 * b.first_poly, b.polys);
        release_owned(ctx, b.slot);
        return r;
    }
    int submit(const uint32_t* d_coef, size_t n, size_t bc, size_t n_c) {
        p1.assign(18 * bc, 0);  // all zero: infinity
        if (!n_c) return KZG_OK;
        const size_t chunk = host_batch_chunk(ctx, bc, n_c);
        int rc = KZG_OK;
        for (size_t at = 0; at < bc && rc == KZG_OK; at += chunk) {
            const size_t polys = bc - at < chunk ? bc - at : chunk;
            int slot = reserve_slot(ctx, lk, false);
            while (slot < 0 && rc == KZG_OK) {
                if (!fifo.empty()) rc = collect_oldest();
                else if ((slot = reserve_slot(ctx, lk, true)) < 0) rc = KZG_ERR_BUSY;
                if (slot < 0 && rc == KZG_OK) slot = reserve_slot(ctx, lk, false);
            }
            if (rc == KZG_OK) rc = commit_batch_submit_locked(ctx, slot, d_coef + 8 * n * at, n_c, polys, n, true);
            if (rc != KZG_OK) {
                if (slot >= 0) release_owned(ctx, slot);
                break;
            }
            fifo.push_back({slot, at, polys});
        }
        return rc;
    }
    int finish(int rc, size_t bc, uint8_t* out48) {
        while (!fifo.empty()) {
            const int r = collect_oldest();
            if (rc == KZG_OK) rc = r;
        }
        if (rc) return rc;
        for (size_t b = 0; b < bc; b++) {
            hf::P1 p;
            std::memcpy(&p, p1.data() + 18 * b, sizeof p);
            hf::p1_compress(out48 + 48 * b, p);
        }
        return KZG_OK;
    }
};
}  // namespace

// sh: null for commitments alone
static int blobs_device(kzg_ctx* ctx, const uint8_t* blobs_be, size_t n, uint32_t lg, size_t batch, size_t stride, const CellsShape* sh,
                        bool bit_reversed, uint8_t* out_commitments, uint8_t* out_cells, uint8_t* out_proofs) {
    std::lock_guard<std::mutex> lkf(ctx->fk20_mu);
    std::unique_lock<std::mutex> lk(ctx->mu);
    if (!ctx->n || !ctx->slots_ready) return KZG_ERR_NO_SRS;
    Fk20Plan pl;
    if (out_proofs && n > sh->l && !fk20_shape(ctx, n, sh->log_l, &pl.m, &pl.log_L)) return KZG_ERR_INVALID_ARG;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    int rc = ensure_ntt(ctx);
    if (rc) return rc;
    const int slot0 = reserve_slot(ctx, lk, true);
    if (slot0 < 0) return KZG_ERR_BUSY;
    SlotLease lease{ctx, slot0};
    Slot& s0 = ctx->slots[slot0];
    const hipStream_t st = s0.stream;
    const size_t N = sh ? sh->N : n, M = sh ? sh->cells : 0;
    size_t chunk = blob_chunk(ctx, n, sh, pl);
    if (chunk > batch) chunk = batch;
    void *wire, *a, *b, *pad = nullptr, *words;
    rc = ctx->blob_ws.get(ctx, kBlobWire, chunk * n * 32, &wire);
    if (rc == KZG_OK) rc = ctx->blob_ws.get(ctx, kBlobA, chunk * N * 32, &a);
    if (rc == KZG_OK) rc = ctx->blob_ws.get(ctx, kBlobB, chunk * N * 32, &b);
    if (rc == KZG_OK && out_cells) rc = ctx->blob_ws.get(ctx, kBlobP, chunk * N * 32, &pad);
    if (rc == KZG_OK) rc = ctx->blob_ws.get(ctx, kBlobWords, (kBlobErrWords + kFk20MaxBatch) * 4, &words);
    if (rc) return rc;
    uint32_t *A = (uint32_t*)a, *B = (uint32_t*)b, *P = (uint32_t*)pad, *err = (uint32_t*)words, *trim = err + kBlobErrWords;
    const Fr30* tw = (const Fr30*)ctx->ntt_tw.p;
    const Fr30 inv_n = fr30_arg_from_mont256(hf::fr_inv(fr_pow2(lg)));
    std::vector<uint32_t> hw(kBlobErrWords + chunk);
    BlobCommits commits{ctx, lk};
    for (size_t b0 = 0; b0 < batch; b0 += chunk) {
        const size_t bc = batch - b0 < chunk ? batch - b0 : chunk;
        // the bytes as they are, decoded into this API's order, interpolated; 1 / n and every n' in one pass
        HIP_TRY(ctx, hipMemsetAsync(err, 0xff, kBlobErrWords * 4, st));
        HIP_TRY(ctx, hipMemsetAsync(trim, 0, bc * 4, st));
        {
            lk.unlock();
            const uint8_t* src = blobs_be + 32 * b0 * stride;
            const hipError_t e = stride > n && bc > 1
                                     ? hipMemcpy2DAsync(wire, n * 32, src, stride * 32, n * 32, bc, hipMemcpyHostToDevice, st)
                                     : hipMemcpyAsync(wire, src, bc * n * 32, hipMemcpyHostToDevice, st);
            lk.lock();
            if (e != hipSuccess) {
                ctx->last_error = std::string("hipMemcpyAsync (blobs): ") + hipGetErrorString(e);
                return KZG_ERR_HIP;
            }
        }
        launch_wire_fr(st, wire, (uint32_t)(bc * n), lg, bit_reversed, A, err);
        uint32_t* coef = const_cast<uint32_t*>(launch_fr_dft(st, A, A, B, lg, bc, tw + 2 * kNttTableLen));
        uint32_t* other = coef == A ? B : A;
        launch_poly_trim(st, coef, (uint32_t)n, n, (uint32_t)bc, &inv_n, trim);
        HIP_TRY(ctx, hipGetLastError());
        HIP_TRY(ctx, hipMemcpyAsync(hw.data(), words, (kBlobErrWords + bc) * 4, hipMemcpyDeviceToHost, st));
        rc = sync_unlocked(ctx, lk, st, "fk20");
        if (rc) return rc;
        if (hw[0] != 0xffffffffu) {
            ctx->last_error = "blobs: polynomial " + std::to_string(b0 + hw[0] / n) + ": value " + std::to_string(hw[0] % n) +
                              " is not below r";
            return KZG_ERR_INVALID_ARG;
        }
        size_t n_max = 0;
        for (size_t i = 0; i < bc; i++) {
            const size_t ne = hw[kBlobErrWords + i];
            if (out_commitments && ne > ctx->n) {
                ctx->last_error = "blobs: polynomial " + std::to_string(b0 + i) + ": n' = " + std::to_string(ne) +
                                  " exceeds the SRS (" + std::to_string(ctx->n) + " points)";
                return KZG_ERR_DEGREE_TOO_HIGH;
            }
            if (out_proofs && ne > sh->l && ne - sh->l > ctx->n) {
                ctx->last_error = "blobs: polynomial " + std::to_string(b0 + i) + ": n' - l = " + std::to_string(ne - sh->l) +
                                  " exceeds the SRS (" + std::to_string(ctx->n) + " points)";
                return KZG_ERR_DEGREE_TOO_HIGH;
            }
            if (ne > n_max) n_max = ne;
        }
        // the stream is idle and the coefficients are resident: the MSMs run on the other slots beside what follows here
        if (out_commitments) rc = commits.submit(coef, n, bc, n_max);
        // (a lambda: a HIP error in here must still reach commits.finish, which collects the sub-batches in flight)
        auto cells = [&]() -> int {
            if (n < N) HIP_TRY(ctx, hipMemsetAsync(P, 0, bc * N * 32, st));
            HIP_TRY(ctx, hipMemcpy2DAsync(P, N * 32, coef, n * 32, n * 32, bc, hipMemcpyDeviceToDevice, st));
            const uint32_t* ev = launch_fr_dft(st, P, P, other, sh->log_n, bc, tw);
            uint32_t* dst = ev == P ? other : P;
            launch_recover_gather(st, ev, dst, sh->log_n, sh->log_l, bc);
            uint32_t* enc = ev == P ? P : other;  // the transform's buffer is free again
            launch_enc_fr(st, dst, (uint32_t)(bc * N), sh->log_l, sh->log_n - sh->log_l, bit_reversed, enc, err + 1);
            HIP_TRY(ctx, hipGetLastError());
            return copy_unlocked(ctx, lk, st, out_cells + 32 * N * b0, enc, bc * N * 32, hipMemcpyDeviceToHost, "hipMemcpyAsync (blobs)");
        };
        if (rc == KZG_OK && out_cells) rc = cells();
        if (rc == KZG_OK && out_proofs) rc = blob_proofs(ctx, lk, s0, coef, n, bc, *sh, bit_reversed, n_max, pl, out_proofs + 48 * M * b0);
        const int r2 = sync_unlocked(ctx, lk, st, "fk20");
        if (rc == KZG_OK) rc = r2;
        if (out_commitments) rc = commits.finish(rc, bc, out_commitments + 48 * b0);
        if (rc) return rc;
    }
    return KZG_OK;
}

static int blobs_entry(kzg_ctx* ctx, const uint8_t* blobs_be, size_t n, size_t batch, size_t stride, bool cells_call,
                       unsigned log_domain, unsigned log_cell, unsigned order, uint8_t* out_commitments, uint8_t* out_cells,
                       uint8_t* out_proofs) {
    if (!ctx) return KZG_ERR_INVALID_ARG;
    auto invalid = [&](const std::string& why) {
        ctx->last_error = "blobs: " + why;
        return KZG_ERR_INVALID_ARG;
    };
    uint32_t lg = 0;
    CellsShape sh;
    if (!ntt_log(n, &lg)) return invalid("n is not a power of two up to 2^KZG_NTT_MAX_LOG");
    if (cells_call && !cells_shape(n, log_domain, log_cell, &sh)) return invalid("unsupported shape (log_domain, log_cell) or n > N");
    if (batch > kMaxCoefficients / (cells_call ? sh.N : n)) return invalid("batch x N does not fit 32 bits");
    if (order != KZG_ORDER_NATURAL && order != KZG_ORDER_BIT_REVERSED)
        return invalid("order is neither KZG_ORDER_NATURAL nor KZG_ORDER_BIT_REVERSED");
    if (batch && (!blobs_be || (cells_call ? !out_proofs : !out_commitments))) return invalid("a required pointer is NULL");
    if (batch > 1 && stride < n) return invalid("stride is below n");
    if (ctx->multi) {
        int rc = KZG_OK;
        kzg_ctx* kid = cells_kid(ctx, &rc);
        return kid ? forwarded(ctx, kid, blobs_entry(kid, blobs_be, n, batch, stride, cells_call, log_domain, log_cell, order,
                                                     out_commitments, out_cells, out_proofs))
                   : rc;
    }
    if (!batch) return KZG_OK;
    return blobs_device(ctx, blobs_be, n, lg, batch, batch > 1 ? stride : n, cells_call ? &sh : nullptr,
                        order == KZG_ORDER_BIT_REVERSED, out_commitments, out_cells, out_proofs);
}

int kzg_blobs_to_commitments_bytes(kzg_ctx* ctx, const uint8_t* blobs_be, size_t n, size_t batch, size_t stride, unsigned order,
                                   uint8_t* out_commitments48) {
    return blobs_entry(ctx, blobs_be, n, batch, stride, false, 0, 0, order, out_commitments48, nullptr, nullptr);
}

int kzg_blobs_to_cells_and_proofs_bytes(kzg_ctx* ctx, const uint8_t* blobs_be, size_t n, size_t batch, size_t stride,
                                        unsigned log_domain, unsigned log_cell, unsigned order, uint8_t* out_commitments48,
                                        uint8_t* out_cells_be, uint8_t* out_proofs48) {
    return blobs_entry(ctx, blobs_be, n, batch, stride, true, log_domain, log_cell, order, out_commitments48, out_cells_be,
                       out_proofs48);
}

// recovery: the received cells decoded on the device in front of recover_host's kernels, the coefficients of the whole batch
// kept in device memory for FK20 (fk20_mu held throughout: the buffer is a workspace of this path)
int kzg_recover_cells_and_proofs_bytes(kzg_ctx* ctx, size_t n, unsigned log_domain, unsigned log_cell, unsigned order,
                                       const uint32_t* cell_ids, size_t k, const uint8_t* cells_be, size_t batch, uint8_t* out_cells_be,
                                       uint8_t* out_proofs48) {
    if (!ctx) return KZG_ERR_INVALID_ARG;
    auto invalid = [&](const std::string& why) {
        ctx->last_error = "recover: " + why;
        return KZG_ERR_INVALID_ARG;
    };
    CellsShape sh;
    if (!cells_shape(n, log_domain, log_cell, &sh)) return invalid("unsupported shape (log_domain, log_cell) or n > N");
    if (log_domain - log_cell > KZG_RECOVER_MAX_LOG_CELLS) return invalid("more than 2^KZG_RECOVER_MAX_LOG_CELLS cells");
    if (n == 0) return invalid("n = 0");
    if (k > sh.cells || k * sh.l < n) return invalid("k l must be at least n, with at most N / l cells");
    if (order != KZG_ORDER_NATURAL && order != KZG_ORDER_BIT_REVERSED)
        return invalid("order is neither KZG_ORDER_NATURAL nor KZG_ORDER_BIT_REVERSED");
    if (!cell_ids || (!cells_be && batch)) return invalid("a required pointer is NULL");
    if (batch > kMaxCoefficients / sh.N) return invalid("batch x N does not fit 32 bits");
    const bool bit_reversed = order == KZG_ORDER_BIT_REVERSED;
    std::vector<int32_t> pos(sh.cells, -1);
    for (size_t t = 0; t < k; t++) {
        if (cell_ids[t] >= sh.cells) return invalid("cell id " + std::to_string(cell_ids[t]) + " is not below N / l");
        // the sampling specs' cell c is this API's cell brp(c) over the N / l cells
        const uint32_t j = bit_reversed ? wire_brp(cell_ids[t], sh.log_n - sh.log_l) : cell_ids[t];
        if (pos[j] >= 0) return invalid("cell id " + std::to_string(cell_ids[t]) + " appears twice");
        pos[j] = (int32_t)t;
    }
    if (ctx->multi) {
        int rc = KZG_OK;
        kzg_ctx* kid = cells_kid(ctx, &rc);
        return kid ? forwarded(ctx, kid, kzg_recover_cells_and_proofs_bytes(kid, n, log_domain, log_cell, order, cell_ids, k, cells_be,
                                                                            batch, out_cells_be, out_proofs48))
                   : rc;
    }
    if (!batch) return KZG_OK;
    std::lock_guard<std::mutex> lkf(ctx->fk20_mu);
    Fk20Plan pl;
    {
        std::lock_guard<std::mutex> lk(ctx->mu);
        if (out_proofs48 && (!ctx->n || !ctx->slots_ready)) return KZG_ERR_NO_SRS;
        if (out_proofs48 && n > sh.l && !fk20_shape(ctx, n, sh.log_l, &pl.m, &pl.log_L)) return KZG_ERR_INVALID_ARG;
        HIP_TRY(ctx, hipSetDevice(ctx->device));
    }
    std::vector<uint32_t> missing;
    for (size_t j = 0; j < sh.cells; j++)
        if (pos[j] < 0) missing.push_back((uint32_t)j);
    RecWire w;
    w.cells_be = cells_be;
    w.bit_reversed = bit_reversed;
    w.ids_sent = cell_ids;
    w.out_cells_be = out_cells_be;
    int rc = ctx->blob_ws.get(ctx, kBlobCoef, batch * n * 32, &w.d_coeffs);  // (fk20_mu guards the workspaces)
    if (rc) return rc;
    rc = recover_host(ctx, sh, n, pos.data(), missing, k, nullptr, batch, nullptr, nullptr, &w);
    if (rc || !out_proofs48) return rc;
    std::unique_lock<std::mutex> lk(ctx->mu);
    if (!ctx->n || !ctx->slots_ready) return KZG_ERR_NO_SRS;  // (the SRS may have gone meanwhile)
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const int slot0 = reserve_slot(ctx, lk, true);
    if (slot0 < 0) return KZG_ERR_BUSY;
    SlotLease lease{ctx, slot0};
    Slot& s0 = ctx->slots[slot0];
    void* words = nullptr;
    rc = ctx->blob_ws.get(ctx, kBlobWords, (kBlobErrWords + kFk20MaxBatch) * 4, &words);
    if (rc) return rc;
    uint32_t* trim = (uint32_t*)words + kBlobErrWords;
    size_t chunk = blob_chunk(ctx, n, &sh, pl);
    if (chunk > batch) chunk = batch;
    std::vector<uint32_t> ht(chunk);
    for (size_t b0 = 0; b0 < batch; b0 += chunk) {
        const size_t bc = batch - b0 < chunk ? batch - b0 : chunk;
        void* coef = (char*)w.d_coeffs + 32 * n * b0;
        HIP_TRY(ctx, hipMemsetAsync(trim, 0, bc * 4, s0.stream));
        launch_poly_trim(s0.stream, coef, (uint32_t)n, n, (uint32_t)bc, nullptr, trim);
        HIP_TRY(ctx, hipGetLastError());
        HIP_TRY(ctx, hipMemcpyAsync(ht.data(), trim, bc * 4, hipMemcpyDeviceToHost, s0.stream));
        rc = sync_unlocked(ctx, lk, s0.stream, "fk20");
        if (rc) return rc;
        size_t n_max = 0;
        for (size_t i = 0; i < bc; i++) {
            if (ht[i] > sh.l && ht[i] - sh.l > ctx->n) {
                ctx->last_error = "recover: polynomial " + std::to_string(b0 + i) + ": n' - l = " + std::to_string(ht[i] - sh.l) +
                                  " exceeds the SRS (" + std::to_string(ctx->n) + " points)";
                return KZG_ERR_DEGREE_TOO_HIGH;
            }
            if (ht[i] > n_max) n_max = ht[i];
        }
        rc = blob_proofs(ctx, lk, s0, coef, n, bc, sh, bit_reversed, n_max, pl, out_proofs48 + 48 * sh.cells * b0);
        if (rc) return rc;
    }
    return KZG_OK;
}

// ---- blob proofs and their Fiat-Shamir challenges (blobproof_kernels.hip, host_sha256.hpp) ----------------
namespace {
// the specs' compute_challenge in two parts: the prefix (domain, degree, the blob bytes as sent), which needs no commitment ...
void challenge_prefix(hf::Sha256& s, const uint8_t* blob_be, size_t n) {
    uint8_t head[32] = {'F', 'S', 'B', 'L', 'O', 'B', 'V', 'E', 'R', 'I', 'F', 'Y', '_', 'V', '1', '_'};
    for (int i = 0; i < 8; i++) head[24 + i] = (uint8_t)((uint64_t)n >> (8 * (7 - i)));  // n as 16 bytes big-endian
    hf::sha256_init(s);
    hf::sha256_update(s, head, 32);
    hf::sha256_update(s, blob_be, n * 32);
}
// ... and the end: the 48 commitment bytes as given, the digest as a big-endian integer, reduced below r (2^256 < 3 r: at most
// two subtractions; about 55 % of digests take one and 9 % two)
void challenge_finish(hf::Sha256 s /* a copy: the prefix stays */, const uint8_t* commitment48, uint8_t out_be[32]) {
    static const uint8_t r_be[32] = {0x73, 0xed, 0xa7, 0x53, 0x29, 0x9d, 0x7d, 0x48, 0x33, 0x39, 0xd8, 0x08, 0x09, 0xa1, 0xd8, 0x05,
                                     0x53, 0xbd, 0xa4, 0x02, 0xff, 0xfe, 0x5b, 0xfe, 0xff, 0xff, 0xff, 0xff, 0x00, 0x00, 0x00, 0x01};
    hf::sha256_update(s, commitment48, 48);
    hf::sha256_final(s, out_be);
    for (int round = 0; round < 2 && std::memcmp(out_be, r_be, 32) >= 0; round++) {
        int borrow = 0;
        for (int i = 31; i >= 0; i--) {
            const int d = (int)out_be[i] - (int)r_be[i] - borrow;
            out_be[i] = (uint8_t)(d & 0xff);
            borrow = d < 0;
        }
    }
}
// work(b) for every b < count on min(count, 16, hardware threads) threads (KZG_HASH_THREADS lowers the 16: measurements), the
// shares interleaved; the caller's thread takes one of them
void hash_pool(size_t count, const std::function<void(size_t)>& work) {
    size_t cap = 16;
    if (const char* v = std::getenv("KZG_HASH_THREADS")) {
        const long k = std::atol(v);
        if (k >= 1 && k < 16) cap = (size_t)k;
    }
    const size_t hw = std::thread::hardware_concurrency();
    size_t nthreads = count < cap ? count : cap;
    if (hw && nthreads > hw) nthreads = hw;
    if (nthreads < 1) nthreads = 1;
    auto share = [&](size_t t) {
        for (size_t b = t; b < count; b += nthreads) work(b);
    };
    std::vector<std::thread> pool;
    for (size_t t = 1; t < nthreads; t++) pool.emplace_back(share, t);
    share(0);
    for (auto& th : pool) th.join();
}
}  // namespace

int kzg_sha256(const uint8_t* data, size_t len, uint8_t out[32]) {
    if (!out || (!data && len)) return KZG_ERR_INVALID_ARG;
    hf::Sha256 s;
    hf::sha256_init(s);
    hf::sha256_update(s, data, len);
    hf::sha256_final(s, out);
    return KZG_OK;
}

int kzg_sha256_pieces(const uint8_t* data, size_t len, size_t piece, int path, uint8_t out[32]) {
    if (!out || (!data && len) || !piece || path < hf::kSha256Auto || path > hf::kSha256ShaNi) return KZG_ERR_INVALID_ARG;
    hf::Sha256 s;
    if (!hf::sha256_init(s, path)) return KZG_ERR_INVALID_ARG;  // the SHA extensions on a CPU without them
    for (size_t at = 0; at < len; at += piece) hf::sha256_update(s, data + at, len - at < piece ? len - at : piece);
    hf::sha256_final(s, out);
    return KZG_OK;
}

int kzg_sha256_has_shani(void) { return hf::sha256_has_shani() ? 1 : 0; }

int kzg_blob_challenges_bytes(const uint8_t* blobs_be, size_t n, size_t batch, size_t stride, const uint8_t* commitments48,
                              uint8_t* out_zs_be) {
    uint32_t lg = 0;
    if (!ntt_log(n, &lg)) return KZG_ERR_INVALID_ARG;
    if (batch && (!blobs_be || !commitments48 || !out_zs_be)) return KZG_ERR_INVALID_ARG;
    if (batch > 1 && stride < n) return KZG_ERR_INVALID_ARG;
    hash_pool(batch, [&](size_t b) {
        hf::Sha256 s;
        challenge_prefix(s, blobs_be + 32 * b * stride, n);
        challenge_finish(s, commitments48 + 48 * b, out_zs_be + 32 * b);
    });
    return KZG_OK;
}

// zs_be: the points (kzg_blobs_open_at_bytes); null: the challenges are derived, from commitments48 when given, else from the
// commitments computed here (kzg_blobs_to_blob_proofs_bytes).  Any of the three outputs but the proofs may be null.
static int blob_openings_device(kzg_ctx* ctx, const uint8_t* blobs_be, size_t n, uint32_t lg, size_t batch, size_t stride,
                                bool bit_reversed, const uint64_t* zs_mont, const uint8_t* commitments48, uint8_t* out_commitments48,
                                uint8_t* out_ys_be, uint8_t* out_proofs48) {
    std::lock_guard<std::mutex> lkf(ctx->fk20_mu);
    std::unique_lock<std::mutex> lk(ctx->mu);
    if (!ctx->n || !ctx->slots_ready) return KZG_ERR_NO_SRS;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    int rc = ensure_ntt(ctx);
    if (rc) return rc;
    const int slot0 = reserve_slot(ctx, lk, true);
    if (slot0 < 0) return KZG_ERR_BUSY;
    SlotLease lease{ctx, slot0};
    Slot& s0 = ctx->slots[slot0];
    const hipStream_t st = s0.stream;
    const bool derive = zs_mont == nullptr, commit = derive && !commitments48;
    const bool single = n <= kBlobProofMaxN;  // the batched kernel; above: the loop of kzg_open_batch
    const Fk20Plan no_plan;
    size_t chunk = blob_chunk(ctx, n, nullptr, no_plan);
    if (chunk > batch) chunk = batch;
    const size_t nq = n - 1;
    void *wire, *a, *b, *zbuf, *words, *flagbuf;
    rc = ctx->blob_ws.get(ctx, kBlobWire, chunk * n * 32, &wire);
    if (rc == KZG_OK) rc = ctx->blob_ws.get(ctx, kBlobA, chunk * n * 32, &a);
    if (rc == KZG_OK) rc = ctx->blob_ws.get(ctx, kBlobB, chunk * n * 32, &b);
    if (rc == KZG_OK) rc = ctx->blob_ws.get(ctx, kBlobP, chunk * kBlobProofZWords * 4, &zbuf);
    if (rc == KZG_OK) rc = ctx->blob_ws.get(ctx, kBlobWords, (kBlobErrWords + kFk20MaxBatch) * 4, &words);
    if (rc == KZG_OK) rc = ctx->blob_ws.get(ctx, kBlobProofs, chunk * 32 * 4, &flagbuf);
    if (rc == KZG_OK && !single) rc = ensure_poly(ctx, s0, n);  // the two-launch scan's scratch
    if (rc) return rc;
    uint32_t *A = (uint32_t*)a, *B = (uint32_t*)b, *err = (uint32_t*)words, *trim = err + kBlobErrWords;
    uint32_t *d_z = (uint32_t*)zbuf, *d_flags = (uint32_t*)flagbuf;
    const Fr30* tw = (const Fr30*)ctx->ntt_tw.p;
    const Fr30 inv_n = fr30_arg_from_mont256(hf::fr_inv(fr_pow2(lg)));
    std::vector<uint32_t> hw(kBlobErrWords + chunk), hz(chunk * kBlobProofZWords), hflags(chunk * 32);
    std::vector<uint8_t> com(48 * chunk), zbe(32);
    std::vector<hf::Sha256> mid(derive ? chunk : 0);
    std::vector<uint64_t> zs_own(derive ? 4 * chunk : 0);
    BlobCommits commits{ctx, lk}, proofs{ctx, lk};
    for (size_t b0 = 0; b0 < batch; b0 += chunk) {
        const size_t bc = batch - b0 < chunk ? batch - b0 : chunk;
        const uint8_t* src = blobs_be + 32 * b0 * stride;
        // the front end of blobs_device: the bytes as they are, decoded, interpolated; 1 / n and every n' in one pass
        HIP_TRY(ctx, hipMemsetAsync(err, 0xff, kBlobErrWords * 4, st));
        HIP_TRY(ctx, hipMemsetAsync(trim, 0, bc * 4, st));
        {
            lk.unlock();
            const hipError_t e = stride > n && bc > 1
                                     ? hipMemcpy2DAsync(wire, n * 32, src, stride * 32, n * 32, bc, hipMemcpyHostToDevice, st)
                                     : hipMemcpyAsync(wire, src, bc * n * 32, hipMemcpyHostToDevice, st);
            lk.lock();
            if (e != hipSuccess) {
                ctx->last_error = std::string("hipMemcpyAsync (blobs): ") + hipGetErrorString(e);
                return KZG_ERR_HIP;
            }
        }
        launch_wire_fr(st, wire, (uint32_t)(bc * n), lg, bit_reversed, A, err);
        uint32_t* coef = const_cast<uint32_t*>(launch_fr_dft(st, A, A, B, lg, bc, tw + 2 * kNttTableLen));
        uint32_t* quot = coef == A ? B : A;  // the transform's other buffer: bc x (n - 1) quotient coefficients fit
        launch_poly_trim(st, coef, (uint32_t)n, n, (uint32_t)bc, &inv_n, trim);
        HIP_TRY(ctx, hipGetLastError());
        HIP_TRY(ctx, hipMemcpyAsync(hw.data(), words, (kBlobErrWords + bc) * 4, hipMemcpyDeviceToHost, st));
        if (derive && !commit) {  // the host hashes while the device decodes and interpolates
            lk.unlock();
            hash_pool(bc, [&](size_t i) { challenge_prefix(mid[i], src + 32 * i * stride, n); });
            lk.lock();
        }
        rc = sync_unlocked(ctx, lk, st, "blob proofs");
        if (rc) return rc;
        if (hw[0] != 0xffffffffu) {
            ctx->last_error = "blob proofs: polynomial " + std::to_string(b0 + hw[0] / n) + ": value " + std::to_string(hw[0] % n) +
                              " is not below r";
            return KZG_ERR_INVALID_ARG;
        }
        size_t n_max = 0;
        for (size_t i = 0; i < bc; i++) {
            const size_t ne = hw[kBlobErrWords + i];
            if (commit && ne > ctx->n) {
                ctx->last_error = "blob proofs: polynomial " + std::to_string(b0 + i) + ": n' = " + std::to_string(ne) +
                                  " exceeds the SRS (" + std::to_string(ctx->n) + " points)";
                return KZG_ERR_DEGREE_TOO_HIGH;
            }
            if (ne > 1 && ne - 1 > ctx->n) {
                ctx->last_error = "blob proofs: polynomial " + std::to_string(b0 + i) + ": n' - 1 = " + std::to_string(ne - 1) +
                                  " exceeds the SRS (" + std::to_string(ctx->n) + " points)";
                return KZG_ERR_DEGREE_TOO_HIGH;
            }
            if (ne > n_max) n_max = ne;
        }
        // the points of this chunk, in the multiplier's form for the kernel
        const uint64_t* zc = zs_mont ? zs_mont + 4 * b0 : zs_own.data();
        if (derive) {
            const uint8_t* cb = commitments48 ? commitments48 + 48 * b0 : com.data();
            if (commit) {  // from the resident coefficients, as kzg_blobs_to_commitments_bytes; the host hashes beside the MSMs
                rc = commits.submit(coef, n, bc, n_max);
                lk.unlock();
                hash_pool(bc, [&](size_t i) { challenge_prefix(mid[i], src + 32 * i * stride, n); });
                lk.lock();
                rc = commits.finish(rc, bc, com.data());
                if (rc) return rc;
            }
            for (size_t i = 0; i < bc; i++) {
                challenge_finish(mid[i], cb + 48 * i, zbe.data());
                (void)wire_fr_host(zbe.data(), zs_own.data() + 4 * i);  // (reduced: below r)
            }
            if (out_commitments48) std::memcpy(out_commitments48 + 48 * b0, cb, 48 * bc);
        }
        std::fill(hz.begin(), hz.end(), 0u);
        for (size_t i = 0; i < bc; i++) {
            hf::Fr z;
            std::memcpy(z.l, zc + 4 * i, 32);
            const Fr30 d = fr30_arg_from_mont256(z);
            std::memcpy(hz.data() + i * kBlobProofZWords, d.d, sizeof d.d);
        }
        // the quotients: one launch for blob sizes, the per-polynomial loop beyond
        s0.timing = ctx->timing;
        std::memset(&s0.times, 0, sizeof s0.times);
        if (single) {
            rc = copy_unlocked(ctx, lk, st, d_z, hz.data(), bc * kBlobProofZWords * 4, hipMemcpyHostToDevice, "hipMemcpyAsync (blob proofs)");
            if (rc) return rc;
            if (s0.timing) HIP_TRY(ctx, hipEventRecord(s0.ev[6], st));
            launch_blobproof_quotients(st, coef, (uint32_t)n, n, (uint32_t)bc, d_z, nq ? quot : nullptr, d_flags);
        } else {
            HIP_TRY(ctx, hipMemsetAsync(d_flags, 0, bc * 32 * 4, st));
            if (s0.timing) HIP_TRY(ctx, hipEventRecord(s0.ev[6], st));
            for (size_t p = 0; p < bc; p++) {
                uint32_t zw[8];
                std::memcpy(zw, zc + 4 * p, 32);
                uint32_t* sm = d_flags + p * 32;
                PolyScratch sc{s0.chunk.dev(), s0.block.dev(), sm, sm + 8};  // scratch re-used in stream order
                launch_quotient(st, coef + p * n * 8, (uint32_t)n, zw, quot + p * nq * 8, sc);
            }
        }
        if (s0.timing) HIP_TRY(ctx, hipEventRecord(s0.ev[7], st));
        HIP_TRY(ctx, hipGetLastError());
        HIP_TRY(ctx, hipMemcpyAsync(hflags.data(), d_flags, bc * 32 * 4, hipMemcpyDeviceToHost, st));
        rc = sync_unlocked(ctx, lk, st, "blob proofs");
        if (rc) return rc;
        if (s0.timing) {
            float ms = 0;
            (void)hipEventElapsedTime(&ms, s0.ev[6], s0.ev[7]);
            s0.times.quotient_ms = ms;
        }
        // the proofs: the batched MSM over the quotients' first n_max - 1 coefficients (the rest are exact zeros)
        rc = proofs.submit(quot, nq, bc, n_max > 1 ? n_max - 1 : 0);
        rc = proofs.finish(rc, bc, out_proofs48 + 48 * b0);
        if (rc) return rc;
        for (size_t i = 0; i < bc; i++) {
            const uint32_t* hs = hflags.data() + 32 * i;
            if (!(hs[0] & 1u)) blob_infinity(out_proofs48 + 48 * (b0 + i), 1);  // n' <= 1: the quotient is zero
            if (out_ys_be) {
                uint64_t y[4];
                std::memcpy(y, hs + 8, 32);
                wire_fr_to_be(y, out_ys_be + 32 * (b0 + i));
            }
        }
    }
    return KZG_OK;
}

static int blob_openings_entry(kzg_ctx* ctx, const uint8_t* blobs_be, size_t n, size_t batch, size_t stride, unsigned order,
                               const uint8_t* zs_be, bool derive, const uint8_t* commitments48, uint8_t* out_commitments48,
                               uint8_t* out_ys_be, uint8_t* out_proofs48) {
    if (!ctx) return KZG_ERR_INVALID_ARG;
    auto invalid = [&](const std::string& why) {
        ctx->last_error = "blob proofs: " + why;
        return KZG_ERR_INVALID_ARG;
    };
    uint32_t lg = 0;
    if (!ntt_log(n, &lg)) return invalid("n is not a power of two up to 2^KZG_NTT_MAX_LOG");
    if (batch > kMaxCoefficients / n) return invalid("batch x n does not fit 32 bits");
    if (order != KZG_ORDER_NATURAL && order != KZG_ORDER_BIT_REVERSED)
        return invalid("order is neither KZG_ORDER_NATURAL nor KZG_ORDER_BIT_REVERSED");
    if (batch && (!blobs_be || !out_proofs48 || (!derive && (!zs_be || !out_ys_be)))) return invalid("a required pointer is NULL");
    if (batch > 1 && stride < n) return invalid("stride is below n");
    if (ctx->multi) {
        int rc = KZG_OK;
        kzg_ctx* kid = cells_kid(ctx, &rc);
        return kid ? forwarded(ctx, kid, blob_openings_entry(kid, blobs_be, n, batch, stride, order, zs_be, derive, commitments48,
                                                             out_commitments48, out_ys_be, out_proofs48))
                   : rc;
    }
    if (!batch) return KZG_OK;
    std::vector<uint64_t> zs;
    if (!derive) {
        zs.resize(4 * batch);
        for (size_t b = 0; b < batch; b++)
            if (!wire_fr_host(zs_be + 32 * b, zs.data() + 4 * b))
                return invalid("polynomial " + std::to_string(b) + ": the point z is not below r");
    }
    return blob_openings_device(ctx, blobs_be, n, lg, batch, batch > 1 ? stride : n, order == KZG_ORDER_BIT_REVERSED,
                                derive ? nullptr : zs.data(), commitments48, out_commitments48, out_ys_be, out_proofs48);
}

int kzg_blobs_open_at_bytes(kzg_ctx* ctx, const uint8_t* blobs_be, size_t n, size_t batch, size_t stride, unsigned order,
                            const uint8_t* zs_be, uint8_t* out_ys_be, uint8_t* out_proofs48) {
    return blob_openings_entry(ctx, blobs_be, n, batch, stride, order, zs_be, false, nullptr, nullptr, out_ys_be, out_proofs48);
}

int kzg_blobs_to_blob_proofs_bytes(kzg_ctx* ctx, const uint8_t* blobs_be, size_t n, size_t batch, size_t stride, unsigned order,
                                   const uint8_t* commitments48, uint8_t* out_commitments48, uint8_t* out_proofs48) {
    return blob_openings_entry(ctx, blobs_be, n, batch, stride, order, nullptr, true, commitments48, out_commitments48, nullptr,
                               out_proofs48);
}

int kzg_verify_blob_proofs_batch_bytes(kzg_ctx* ctx, const uint8_t* blobs_be, size_t n, size_t batch, size_t stride, unsigned order,
                                       const uint8_t* commitments48, const uint8_t* proofs48, const void* setup_g2,
                                       size_t g2_stride_bytes, int* valid) {
    // the challenges first, where the inputs can be hashed at all; what cannot is refused by the sibling below, in its own words
    // (the points it is handed are then never read)
    uint32_t lg = 0;
    std::vector<uint8_t> zs(32 * (batch && batch <= KZG_VERIFY_MAX_OPENINGS ? batch : 1));
    if (ctx && batch && batch <= KZG_VERIFY_MAX_OPENINGS && ntt_log(n, &lg) && blobs_be && commitments48 && !(batch > 1 && stride < n))
        (void)kzg_blob_challenges_bytes(blobs_be, n, batch, batch > 1 ? stride : n, commitments48, zs.data());
    const BlobWire w = {blobs_be, order, commitments48, zs.data(), proofs48, nullptr};
    return verify_evaluations_impl(ctx, nullptr, n, batch, stride, nullptr, nullptr, nullptr, setup_g2, g2_stride_bytes, nullptr,
                                   valid, &w);
}

// the encoders on their own: building blocks and test hooks; they need no SRS
int kzg_g1_compress_batch(kzg_ctx* ctx, const uint64_t* in_p1, size_t n, uint8_t* out48) {
    if (!ctx) return KZG_ERR_INVALID_ARG;
    if (n > kMaxCoefficients - 1 || (n && (!in_p1 || !out48))) {
        ctx->last_error = "g1 compress: a required pointer is NULL or n does not fit 32 bits";
        return KZG_ERR_INVALID_ARG;
    }
    if (!n) return KZG_OK;
    if (ctx->multi) {
        kzg_ctx* kid = multi_kid(ctx->multi, 0);
        return forwarded(ctx, kid, kzg_g1_compress_batch(kid, in_p1, n, out48));
    }
    std::lock_guard<std::mutex> lkf(ctx->fk20_mu);
    std::unique_lock<std::mutex> lk(ctx->mu);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const int slot = reserve_slot(ctx, lk, true);
    if (slot < 0) return KZG_ERR_BUSY;
    SlotLease lease{ctx, slot};
    Slot& s = ctx->slots[slot];
    int rc = ensure_slot_basics(ctx, s);
    void *jac = nullptr, *aff = nullptr, *prefix = nullptr, *enc = nullptr;
    if (rc == KZG_OK) rc = ctx->blob_ws.get(ctx, kBlobP1, n * 144, &jac);
    if (rc == KZG_OK) rc = ctx->blob_ws.get(ctx, kBlobA, n * kAffineBytes, &aff);
    if (rc == KZG_OK) rc = ctx->blob_ws.get(ctx, kBlobB, n * 64, &prefix);
    if (rc == KZG_OK) rc = ctx->blob_ws.get(ctx, kBlobProofs, n * 48, &enc);
    if (rc) return rc;
    const hipStream_t st = s.stream;
    rc = copy_unlocked(ctx, lk, st, jac, in_p1, n * 144, hipMemcpyHostToDevice, "hipMemcpyAsync (blobs)");
    if (rc) return rc;
    launch_jacobian_to_affine(st, jac, (uint32_t)n, aff, prefix);
    launch_enc_g1(st, aff, (uint32_t)n, 0, false, enc);
    HIP_TRY(ctx, hipGetLastError());
    rc = copy_unlocked(ctx, lk, st, out48, enc, n * 48, hipMemcpyDeviceToHost, "hipMemcpyAsync (blobs)");
    const int r2 = sync_unlocked(ctx, lk, st, "fk20");
    return rc ? rc : r2;
}

int kzg_fr_to_bytes_batch(kzg_ctx* ctx, const uint64_t* in_fr_mont, size_t n, uint8_t* out32_be, size_t* bad_index) {
    if (!ctx) return KZG_ERR_INVALID_ARG;
    if (bad_index) *bad_index = (size_t)-1;
    if (n > kMaxCoefficients - 1 || (n && (!in_fr_mont || !out32_be))) {
        ctx->last_error = "fr to bytes: a required pointer is NULL or n does not fit 32 bits";
        return KZG_ERR_INVALID_ARG;
    }
    if (!n) return KZG_OK;
    if (ctx->multi) {
        kzg_ctx* kid = multi_kid(ctx->multi, 0);
        return forwarded(ctx, kid, kzg_fr_to_bytes_batch(kid, in_fr_mont, n, out32_be, bad_index));
    }
    std::lock_guard<std::mutex> lkf(ctx->fk20_mu);
    std::unique_lock<std::mutex> lk(ctx->mu);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const int slot = reserve_slot(ctx, lk, true);
    if (slot < 0) return KZG_ERR_BUSY;
    SlotLease lease{ctx, slot};
    Slot& s = ctx->slots[slot];
    int rc = ensure_slot_basics(ctx, s);
    void *vals = nullptr, *enc = nullptr, *words = nullptr;
    if (rc == KZG_OK) rc = ctx->blob_ws.get(ctx, kBlobA, n * 32, &vals);
    if (rc == KZG_OK) rc = ctx->blob_ws.get(ctx, kBlobB, n * 32, &enc);
    if (rc == KZG_OK) rc = ctx->blob_ws.get(ctx, kBlobWords, (kBlobErrWords + kFk20MaxBatch) * 4, &words);
    if (rc) return rc;
    const hipStream_t st = s.stream;
    uint32_t* err = (uint32_t*)words;
    HIP_TRY(ctx, hipMemsetAsync(err, 0xff, kBlobErrWords * 4, st));
    rc = copy_unlocked(ctx, lk, st, vals, in_fr_mont, n * 32, hipMemcpyHostToDevice, "hipMemcpyAsync (blobs)");
    if (rc) return rc;
    launch_enc_fr(st, vals, (uint32_t)n, 0, 0, false, enc, err);
    HIP_TRY(ctx, hipGetLastError());
    uint32_t herr = 0;
    HIP_TRY(ctx, hipMemcpyAsync(&herr, err, 4, hipMemcpyDeviceToHost, st));
    rc = copy_unlocked(ctx, lk, st, out32_be, enc, n * 32, hipMemcpyDeviceToHost, "hipMemcpyAsync (blobs)");
    const int r2 = sync_unlocked(ctx, lk, st, "fk20");
    if (rc || r2) return rc ? rc : r2;
    if (herr != 0xffffffffu) {
        if (bad_index) *bad_index = herr;
        ctx->last_error = "fr to bytes: value " + std::to_string(herr) + " is not below r";
        return KZG_ERR_INVALID_ARG;
    }
    return KZG_OK;
}

// ---- raw device memory -----------------------------------------------------------------------

int kzg_dev_alloc(kzg_ctx* ctx, size_t bytes, void** out) {
    KZG_SINGLE_DEVICE_ONLY(ctx);
    if (!ctx || !out) return KZG_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(ctx->mu);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipMalloc(out, bytes ? bytes : 1));
    return KZG_OK;
}
int kzg_dev_free(kzg_ctx* ctx, void* p) {
    KZG_SINGLE_DEVICE_ONLY(ctx);
    if (!ctx) return KZG_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(ctx->mu);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipFree(p));
    return KZG_OK;
}
int kzg_dev_upload(kzg_ctx* ctx, void* dst, const void* src, size_t bytes) {
    KZG_SINGLE_DEVICE_ONLY(ctx);
    if (!ctx || (!dst && bytes) || (!src && bytes)) return KZG_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(ctx->mu);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice));
    return KZG_OK;
}
int kzg_dev_download(kzg_ctx* ctx, void* dst, const void* src, size_t bytes) {
    KZG_SINGLE_DEVICE_ONLY(ctx);
    if (!ctx || (!dst && bytes) || (!src && bytes)) return KZG_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(ctx->mu);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost));
    return KZG_OK;
}

// ---- host-side G1 helpers ----------------------------------------------------------------------

int kzg_g1_sum(const uint64_t* p1s, size_t k, uint64_t out_p1[18]) {
    if (!out_p1 || (!p1s && k)) return KZG_ERR_INVALID_ARG;
    hf::P1 acc = hf::p1_inf();
    for (size_t i = 0; i < k; i++) {
        hf::P1 p;
        std::memcpy(&p, p1s + 18 * i, sizeof p);
        acc = hf::p1_add(acc, p);
    }
    write_p1(out_p1, hf::p1_normalize(acc));
    return KZG_OK;
}

int kzg_g1_compress(const uint64_t p1[18], uint8_t out[48]) {
    if (!p1 || !out) return KZG_ERR_INVALID_ARG;
    hf::P1 p;
    std::memcpy(&p, p1, sizeof p);
    hf::p1_compress(out, p);
    return KZG_OK;
}

int kzg_g1_uncompress(const uint8_t in[48], uint64_t out_p1[18]) {
    if (!in || !out_p1) return KZG_ERR_INVALID_ARG;
    hf::P1 p;
    if (!hf::p1_uncompress(p, in)) return KZG_ERR_INVALID_ARG;
    write_p1(out_p1, p);
    return KZG_OK;
}

int kzg_verify_proof(const uint64_t commitment_p1[18], const uint64_t proof_p1[18], const uint64_t z[4],
                     const uint64_t y[4], const uint64_t s_g2_p2[36], int* valid) {
    if (!commitment_p1 || !proof_p1 || !z || !y || !s_g2_p2 || !valid) return KZG_ERR_INVALID_ARG;
    int r = hf::verify_proof(commitment_p1, proof_p1, z, y, s_g2_p2);
    if (r < 0) return KZG_ERR_INVALID_ARG;
    *valid = r;
    return KZG_OK;
}

int kzg_verify_proof_batch(const uint64_t* commitments_p1, const uint64_t* proofs_p1, const uint64_t* zs,
                           const uint64_t* ys, const uint64_t s_g2_p2[36], size_t n, int* valid) {
    if ((!commitments_p1 || !proofs_p1 || !zs || !ys || !valid) && n) return KZG_ERR_INVALID_ARG;
    if (!s_g2_p2) return KZG_ERR_INVALID_ARG;
    size_t nthreads = std::thread::hardware_concurrency();
    if (nthreads == 0) nthreads = 1;
    if (nthreads > n) nthreads = n;
    std::vector<int> results(n, 0);
    auto work = [&](size_t t) {
        for (size_t i = t; i < n; i += nthreads)
            results[i] = hf::verify_proof(commitments_p1 + 18 * i, proofs_p1 + 18 * i, zs + 4 * i, ys + 4 * i, s_g2_p2);
    };
    if (nthreads <= 1) {
        if (n) work(0);
    } else {
        std::vector<std::thread> pool;
        for (size_t t = 1; t < nthreads; t++) pool.emplace_back(work, t);
        work(0);
        for (auto& th : pool) th.join();
    }
    for (size_t i = 0; i < n; i++) {
        if (results[i] < 0) return KZG_ERR_INVALID_ARG;
        valid[i] = results[i];
    }
    return KZG_OK;
}

// ---- combined openings, the verifier's side (host only) ---------------------------------------
// C = sum gamma^i C_i and y = sum gamma^i y_i by Horner in gamma: t - 1 scalar multiplications.  With several threads the
// list is cut into runs of L commitments, every run is a Horner sum of its own and the run totals are joined by Horner in
// gamma^L -- still t - 1 multiplications, of which about L + t / L lie on the critical path; the thread count is therefore
// the one nearest sqrt(t), capped by min(hardware threads, t) as in kzg_verify_proof_batch.
int kzg_combine_claims(const uint64_t* commitments_p1, const uint64_t* ys, size_t t, const uint64_t gamma[4],
                       uint64_t out_commitment_p1[18], uint64_t out_y[4]) {
    if (!commitments_p1 || !ys || !gamma || !out_commitment_p1 || !out_y) return KZG_ERR_INVALID_ARG;
    if (t < 1 || t > KZG_MAX_COMBINE) return KZG_ERR_INVALID_ARG;
    hf::Fr g, v;
    std::memcpy(g.l, gamma, 32);
    if (hf::fr_geq(g, hf::kFrMod)) return KZG_ERR_INVALID_ARG;
    for (size_t i = 0; i < t; i++) {
        std::memcpy(v.l, ys + 4 * i, 32);
        if (hf::fr_geq(v, hf::kFrMod)) return KZG_ERR_INVALID_ARG;
    }
    hf::Fr y;
    std::memcpy(y.l, ys + 4 * (t - 1), 32);
    for (size_t i = t - 1; i-- > 0;) {
        std::memcpy(v.l, ys + 4 * i, 32);
        y = hf::fr_add(hf::fr_mul(y, g), v);
    }
    size_t cap = std::thread::hardware_concurrency();
    if (cap == 0) cap = 1;
    if (cap > t) cap = t;
    size_t nthreads = 1;
    while ((nthreads + 1) * (nthreads + 1) <= t && nthreads < cap) nthreads++;
    const size_t L = (t + nthreads - 1) / nthreads;  // commitments per run
    const size_t runs = (t + L - 1) / L;
    auto load = [&](size_t i) {
        hf::P1 p;
        std::memcpy(&p, commitments_p1 + 18 * i, sizeof p);
        return p;
    };
    auto horner = [&](size_t lo, size_t hi, const uint64_t k[4]) {  // sum_{lo <= i < hi} gamma^(i - lo) C_i
        hf::P1 acc = load(hi - 1);
        for (size_t i = hi - 1; i-- > lo;) acc = hf::p1_add(hf::p1_mul(acc, k), load(i));
        return acc;
    };
    uint64_t gk[4];
    hf::fr_from_mont(g.l, gk);
    std::vector<hf::P1> part(runs);
    auto work = [&](size_t r) { part[r] = horner(r * L, std::min(t, (r + 1) * L), gk); };
    if (runs <= 1) {
        work(0);
    } else {
        std::vector<std::thread> pool;
        for (size_t r = 1; r < runs; r++) pool.emplace_back(work, r);
        work(0);
        for (auto& th : pool) th.join();
    }
    hf::P1 acc = part[runs - 1];
    if (runs > 1) {
        uint64_t gl[4];
        const hf::Fr gL = hf::fr_pow(g, L);
        hf::fr_from_mont(gL.l, gl);
        for (size_t r = runs - 1; r-- > 0;) acc = hf::p1_add(hf::p1_mul(acc, gl), part[r]);
    }
    write_p1(out_commitment_p1, hf::p1_normalize(acc));
    std::memcpy(out_y, y.l, 32);
    return KZG_OK;
}

int kzg_verify_combined(const uint64_t* commitments_p1, const uint64_t* ys, size_t t, const uint64_t z[4], const uint64_t gamma[4],
                        const uint64_t proof_p1[18], const uint64_t s_g2[36], int* valid) {
    if (!z || !proof_p1 || !s_g2 || !valid) return KZG_ERR_INVALID_ARG;
    uint64_t c[18], y[4];
    const int rc = kzg_combine_claims(commitments_p1, ys, t, gamma, c, y);
    if (rc) return rc;
    return kzg_verify_proof(c, proof_p1, z, y, s_g2, valid);
}

// Openings at several point sets, the verifier's side (host only): the sets are checked as the prover
// checks them, every set's commitments and values are folded with the powers of gamma (t scalar multiplications), and
// hf::verify_sets runs the pairing check.
int kzg_verify_sets(const uint64_t* commitments_p1, size_t t, const uint32_t* set_of, const uint32_t* set_len, size_t m,
                    const uint64_t* zs, const uint64_t* ys, const uint64_t gamma[4], const uint64_t proof_p1[18],
                    const void* setup_g1, size_t g1_stride_bytes, const void* setup_g2, size_t g2_stride_bytes, int* valid) {
    if (!commitments_p1 || !set_of || !set_len || !zs || !ys || !gamma || !proof_p1 || !setup_g1 || !setup_g2 || !valid)
        return KZG_ERR_INVALID_ARG;
    if (t < 1 || t > KZG_MAX_COMBINE || m < 1 || m > KZG_MAX_SETS) return KZG_ERR_INVALID_ARG;
    SetsPlan plan;
    std::string why;
    if (!sets_plan(plan, why, t, set_of, set_len, m, zs, gamma)) return KZG_ERR_INVALID_ARG;
    std::vector<hf::SetCheck> sets(m);
    for (size_t g = 0; g < m; g++) {
        sets[g].k = plan.set_len[g];
        for (size_t j = 0; j < sets[g].k; j++) {
            sets[g].z[j] = plan.pts[plan.pt_of[g][j]];
            sets[g].v[j] = hf::Fr{{0, 0, 0, 0}};
        }
        sets[g].c = hf::p1_inf();
    }
    hf::Fr gp = hf::kFrOne;
    for (size_t i = 0; i < t; i++) {
        hf::SetCheck& S = sets[set_of[i]];
        for (size_t j = 0; j < S.k; j++) {
            hf::Fr y;
            if (!fr_arg_below_r(ys + 4 * (plan.val_first[i] + j), &y)) return KZG_ERR_INVALID_ARG;
            S.v[j] = hf::fr_add(S.v[j], hf::fr_mul(gp, y));
        }
        hf::P1 c;
        std::memcpy(&c, commitments_p1 + 18 * i, sizeof c);
        if (!hf::p1_on_curve(c)) return KZG_ERR_INVALID_ARG;
        uint64_t e[4];
        hf::fr_from_mont(gp.l, e);
        S.c = hf::p1_add(S.c, hf::p1_mul(c, e));
        gp = hf::fr_mul(gp, plan.gamma);
    }
    const int r = hf::verify_sets(sets.data(), m, plan.pts, plan.npts, proof_p1, (const uint8_t*)setup_g1, g1_stride_bytes,
                                  (const uint8_t*)setup_g2, g2_stride_bytes);
    if (r < 0) return KZG_ERR_INVALID_ARG;
    *valid = r;
    return KZG_OK;
}

// The last round of a circuit's proof, the verifier's side (host only): PI(zeta) from the public inputs
// with one batch inversion, [r] = sum scalar commitment + konst G1 from the key, [z] and [T_c] with the scalars the prover put on
// the coefficients (lin_scalars), then kzg_verify_sets over [ [r] | wires | sigma_0 .. sigma_(t-2) | [z] ] with the values
// [ 0 | abar | sbar | z(zeta w) ].
namespace {
// the lookup of a proof (section 4.26), the verifier's side: c table columns, theta, [m] and [phi]; the key then has 2 t + c + 3
// commitments and the evaluations go on with tbar_0 .. tbar_(c-1), qbar, phi(zeta w)
struct LookupClaim {
    size_t c;
    const uint64_t *theta, *m_p1, *phi_p1;
};
// the custom gates of a proof (section 4.27), the verifier's side: g terms and their g x t exponents; the key then has 2 t + 2 + g
// commitments, the proof's fields are the plain proof's
// A next-row proof (section 4.28) adds the second matrix and the rho values f_j(zeta w), j in R ascending
struct CustomClaim {
    size_t g;
    const uint8_t* exps;
    const uint8_t* exps_next = nullptr;
    const uint64_t* evals_next = nullptr;
};
int circuit_verify_impl(const uint64_t* key_p1s, size_t n, size_t t, unsigned log_ext, const uint64_t* shifts, const uint64_t* wire_p1s,
                        const uint64_t z_p1[18], const uint64_t* t_p1s, const uint64_t* public_inputs, size_t n_public,
                        const uint64_t* evals, const uint64_t alpha[4], const uint64_t beta[4], const uint64_t gamma[4],
                        const uint64_t zeta[4], const uint64_t v[4], const uint64_t proof_p1[18], const void* setup_g1,
                        size_t g1_stride_bytes, const void* setup_g2, size_t g2_stride_bytes, int* valid, const LookupClaim* lookup,
                        const CustomClaim* custom = nullptr);
// PI(zeta) = sum_i PI_i L_i(zeta), L_i(zeta) = w^i (zeta^n - 1) / (n (zeta - w^i)), with one batch inversion beside 1 / n;
// zeta = w^k: L_i(zeta) = [i = k].  Zero without public inputs
hf::Fr public_input_at(const hf::Fr& zeta, size_t n, uint32_t lg_n, const hf::Fr* pub, size_t n_public) {
    hf::Fr pi_zeta = kFrZero;
    if (!n_public) return pi_zeta;
    const hf::Fr w = hf::fr_domain_root(lg_n);
    std::vector<hf::Fr> wi(n_public), den(n_public), pre(n_public);
    hf::Fr cur = hf::kFrOne, run = hf::kFrOne;
    size_t on_h = n_public;
    for (size_t i = 0; i < n_public; i++) {
        wi[i] = cur;
        den[i] = hf::fr_sub(zeta, cur);
        if (fr_equal(den[i], kFrZero)) on_h = i;
        pre[i] = run;  // the product of the denominators before i
        run = hf::fr_mul(run, den[i]);
        cur = hf::fr_mul(cur, w);
    }
    if (on_h < n_public) return pub[on_h];
    hf::Fr inv = hf::fr_inv(run);
    for (size_t i = n_public; i-- > 0;) {
        pi_zeta = hf::fr_add(pi_zeta, hf::fr_mul(hf::fr_mul(pub[i], wi[i]), hf::fr_mul(inv, pre[i])));
        inv = hf::fr_mul(inv, den[i]);
    }
    const hf::Fr Z = hf::fr_sub(hf::fr_pow(zeta, n), hf::kFrOne);
    return hf::fr_mul(pi_zeta, hf::fr_mul(Z, hf::fr_inv(fr_pow2(lg_n))));
}
}  // namespace

int kzg_circuit_verify(const uint64_t* key_p1s, size_t n, size_t t, unsigned log_ext, const uint64_t* shifts, const uint64_t* wire_p1s,
                       const uint64_t z_p1[18], const uint64_t* t_p1s, const uint64_t* public_inputs, size_t n_public,
                       const uint64_t* evals, const uint64_t alpha[4], const uint64_t beta[4], const uint64_t gamma[4],
                       const uint64_t zeta[4], const uint64_t v[4], const uint64_t proof_p1[18], const void* setup_g1,
                       size_t g1_stride_bytes, const void* setup_g2, size_t g2_stride_bytes, int* valid) {
    return circuit_verify_impl(key_p1s, n, t, log_ext, shifts, wire_p1s, z_p1, t_p1s, public_inputs, n_public, evals, alpha, beta, gamma,
                               zeta, v, proof_p1, setup_g1, g1_stride_bytes, setup_g2, g2_stride_bytes, valid, nullptr);
}

namespace {
// kzg_circuit_verify; with a lookup claim the verifier of section 4.26: [r_L] and the stack's c + 2 more entries
int circuit_verify_impl(const uint64_t* key_p1s, size_t n, size_t t, unsigned log_ext, const uint64_t* shifts, const uint64_t* wire_p1s,
                        const uint64_t z_p1[18], const uint64_t* t_p1s, const uint64_t* public_inputs, size_t n_public,
                        const uint64_t* evals, const uint64_t alpha[4], const uint64_t beta[4], const uint64_t gamma[4],
                        const uint64_t zeta[4], const uint64_t v[4], const uint64_t proof_p1[18], const void* setup_g1,
                        size_t g1_stride_bytes, const void* setup_g2, size_t g2_stride_bytes, int* valid, const LookupClaim* lookup,
                        const CustomClaim* custom) {
    if (!key_p1s || !shifts || !wire_p1s || !z_p1 || !t_p1s || (!public_inputs && n_public) || !evals || !alpha || !beta || !gamma ||
        !zeta || !v || !proof_p1 || !setup_g1 || !setup_g2 || !valid)
        return KZG_ERR_INVALID_ARG;
    PqShape sh;
    if (log_ext > kPqMaxLogExt || !pq_shape(n, (size_t)1 << log_ext, &sh) || t < KZG_CIRCUIT_MIN_COLUMNS || t > kPqMaxColumns ||
        t + 1 > sh.rot || n_public > n)
        return KZG_ERR_INVALID_ARG;
    const size_t lc = lookup ? lookup->c : 0;
    if (lookup && !lookup_shape_ok(t, sh.rot, lc)) return KZG_ERR_INVALID_ARG;
    if (custom && (lookup || (!custom->exps_next && !custom_shape_ok(t, sh.rot, custom->g, custom->exps, nullptr))))
        return KZG_ERR_INVALID_ARG;
    uint8_t next_wires[kPqMaxColumns] = {};
    const size_t rho = custom && custom->exps_next
                           ? next_shape_rho(n, t, sh.rot, custom->g, custom->exps, custom->exps_next, nullptr, next_wires) : 0;
    if (custom && custom->exps_next && (!rho || !custom->evals_next)) return KZG_ERR_INVALID_ARG;
    const size_t e = sh.rot, npoly = 2 * t + 1 + (lookup ? lc + 2 : 0);
    LinChallenges ch;
    hf::Fr vf;
    if (!fr_arg_below_r(alpha, &ch.alpha) || !fr_arg_below_r(beta, &ch.beta) || !fr_arg_below_r(gamma, &ch.gamma) ||
        !fr_arg_below_r(zeta, &ch.zeta) || !fr_arg_below_r(v, &vf))
        return KZG_ERR_INVALID_ARG;
    std::vector<hf::Fr> ys(npoly, kFrZero), pub(n_public), ks(t);  // the stack's values: 0, abar, sbar, z(zeta w)
    for (size_t i = 1; i < npoly; i++)
        if (!fr_arg_below_r(evals + 4 * (i - 1), &ys[i])) return KZG_ERR_INVALID_ARG;
    std::vector<hf::Fr> ys_next(rho);  // the second value of a wire of R, at zeta w
    for (size_t k = 0; k < rho; k++)
        if (!fr_arg_below_r(custom->evals_next + 4 * k, &ys_next[k])) return KZG_ERR_INVALID_ARG;
    for (size_t i = 0; i < n_public; i++)
        if (!fr_arg_below_r(public_inputs + 4 * i, &pub[i])) return KZG_ERR_INVALID_ARG;
    for (size_t j = 0; j < t; j++)
        if (!fr_arg_below_r(shifts + 4 * j, &ks[j])) return KZG_ERR_INVALID_ARG;
    auto load = [](const uint64_t* p, hf::P1* out) {
        std::memcpy(out, p, sizeof *out);
        return hf::p1_on_curve(*out);
    };
    // the commitments r is made of, in lin_scalars' order
    std::vector<hf::P1> cs(t + e + 3);
    bool on_curve = true;
    for (size_t j = 0; j < t + 2; j++) on_curve = load(key_p1s + 18 * j, &cs[j]) && on_curve;
    on_curve = load(z_p1, &cs[t + 2]) && on_curve;
    on_curve = load(key_p1s + 18 * (2 * t + 1), &cs[t + 3]) && on_curve;
    for (size_t k = 0; k + 1 < e; k++) on_curve = load(t_p1s + 18 * k, &cs[t + 4 + k]) && on_curve;
    hf::P1 tmp;
    for (size_t j = 0; j < t; j++) on_curve = load(wire_p1s + 18 * j, &tmp) && load(key_p1s + 18 * (t + 2 + j), &tmp) && on_curve;
    hf::Fr theta = kFrZero;
    if (lookup) {  // [phi] and [m] follow r's other commitments; the table's commitments are checked like the sigmas'
        cs.resize(t + e + 5);
        on_curve = load(lookup->phi_p1, &cs[t + e + 3]) && load(lookup->m_p1, &cs[t + e + 4]) && on_curve;
        for (size_t j = 0; j < lc + 1; j++) on_curve = load(key_p1s + 18 * (2 * t + 2 + j), &tmp) && on_curve;
        if (!fr_arg_below_r(lookup->theta, &theta)) return KZG_ERR_INVALID_ARG;
    }
    if (custom) {  // [qx_s] follow r's other commitments
        cs.resize(t + e + 3 + custom->g);
        for (size_t k = 0; k < custom->g; k++) on_curve = load(key_p1s + 18 * (2 * t + 2 + k), &cs[t + e + 3 + k]) && on_curve;
    }
    if (!on_curve) return KZG_ERR_INVALID_ARG;
    // PI(zeta) = sum_i PI_i L_i(zeta), L_i(zeta) = w^i (zeta^n - 1) / (n (zeta - w^i)); zeta = w^k: L_i(zeta) = [i = k]
    const hf::Fr pi_zeta = public_input_at(ch.zeta, n, sh.lg_n, pub.data(), n_public);
    hf::Fr konst;
    std::vector<hf::Fr> sc;
    lin_scalars(n, sh.lg_n, t, e, shifts, ch, &ys[1], &ys[1 + t], ys[2 * t], pi_zeta, &sc, &konst);
    if (lookup) {
        const LookupLin ll = lookup_lin(n, sh.lg_n, lc, ch, theta, &ys[1], &ys[2 * t + 1], ys[2 * t + 1 + lc], ys[2 * t + 2 + lc]);
        sc.push_back(ll.on_phi);
        sc.push_back(ll.on_m);
        konst = hf::fr_add(konst, ll.konst);
    }
    if (custom) {
        std::vector<hf::Fr> cx;
        custom_lin_scalars(t, custom->g, custom->exps, &ys[1], &cx, custom->exps_next, rho, next_wires, ys_next.data());
        sc.insert(sc.end(), cx.begin(), cx.end());
    }
    auto times = [](const hf::P1& p, const hf::Fr& k) {  // the scalar multiplication of kzg_combine_claims
        uint64_t plain[4];
        hf::fr_from_mont(k.l, plain);
        return hf::p1_mul(p, plain);
    };
    hf::P1 r = times(hf::p1_generator(), konst);
    for (size_t k = 0; k < cs.size(); k++) r = hf::p1_add(r, times(cs[k], sc[k]));
    r = hf::p1_normalize(r);
    // the stack, its sets and values
    std::vector<uint64_t> stack(18 * npoly), yl(4 * (npoly + rho));
    std::memcpy(stack.data(), &r, sizeof r);
    std::memcpy(stack.data() + 18, wire_p1s, 18 * 8 * t);
    std::memcpy(stack.data() + 18 * (1 + t), key_p1s + 18 * (t + 2), 18 * 8 * (t - 1));
    std::memcpy(stack.data() + 18 * 2 * t, z_p1, 18 * 8);
    if (lookup) {
        std::memcpy(stack.data() + 18 * (2 * t + 1), key_p1s + 18 * (2 * t + 2), 18 * 8 * (lc + 1));
        std::memcpy(stack.data() + 18 * (2 * t + 2 + lc), lookup->phi_p1, 18 * 8);
    }
    // a next-row proof: the wires of R on a third set {zeta, zeta w}, two values each, in the set's order
    std::vector<uint32_t> set_of(npoly, 0);
    set_of[2 * t] = 1;
    set_of[npoly - 1] = 1;
    for (size_t k = 0; k < rho; k++) set_of[1 + next_wires[k]] = 2;
    for (size_t i = 0, at = 0, k = 0; i < npoly; i++) {
        std::memcpy(yl.data() + 4 * at++, ys[i].l, 32);
        if (set_of[i] == 2) std::memcpy(yl.data() + 4 * at++, ys_next[k++].l, 32);
    }
    const uint32_t set_len[3] = {1, 1, 2};
    const hf::Fr zeta_w = hf::fr_mul(ch.zeta, hf::fr_domain_root(sh.lg_n));
    uint64_t zs[16];
    std::memcpy(zs, ch.zeta.l, 32);
    std::memcpy(zs + 4, zeta_w.l, 32);
    std::memcpy(zs + 8, zs, 64);
    return kzg_verify_sets(stack.data(), npoly, set_of.data(), set_len, rho ? 3 : 2, zs, yl.data(), v, proof_p1, setup_g1, g1_stride_bytes,
                           setup_g2, g2_stride_bytes, valid);
}
}  // namespace

// ---- a circuit's proof as bytes: the hashed transcript and the proof formats (host only) -----------------
// The four formats (plain; custom gates, section 4.27; next-row gates, 4.28; lookup, 4.26) are instances of one description, ProofSpec:
//   h0 = SHA256(DST | header | shifts | exponents (custom kinds) | the nkey key commitments | public inputs)
//   the proof is a list of segments; h_(i+1) = SHA256(h_i | segment i), after which that segment's challenges are drawn,
//   fr(SHA256(h_(i+1) | 00)) and, for a second one, fr(SHA256(h_(i+1) | 01))
//   kind     DST                              header (u64be)                 nkey           nevals
//   plain    kzg_mi355x/plonk/v1              n, t, log_ext, n_public        2 t + 2        2 t
//   custom   kzg_mi355x/plonk-custom/v1       n, t, log_ext, g, n_public     2 t + 2 + g    2 t
//   next     kzg_mi355x/plonk-custom-next/v1  n, t, log_ext, g, n_public     2 t + 2 + g    2 t + rho
//   lookup   kzg_mi355x/plonk-lookup/v1       n, t, log_ext, c, n_public     2 t + c + 3    2 t + c + 2
//   segments, plain family:  wires -> beta, gamma | [z] -> alpha | [T_0] .. [T_(e-2)] -> zeta | evaluations -> v | W
//   segments, lookup:        wires -> theta | [m] -> beta, gamma | [z] [phi] -> alpha | chunks -> zeta | evaluations -> v | W
// scalars as 32 big-endian canonical bytes, points as 48 compressed bytes, fr(d) = d read big-endian mod r.
namespace {
constexpr char kProofDst[] = "kzg_mi355x/plonk/v1";  // each hashed without the terminator
constexpr char kCustomProofDst[] = "kzg_mi355x/plonk-custom/v1";
constexpr char kNextProofDst[] = "kzg_mi355x/plonk-custom-next/v1";
constexpr char kLookupProofDst[] = "kzg_mi355x/plonk-lookup/v1";

void proof_fr_to_be(const hf::Fr& mont, uint8_t out[32]) {
    uint64_t plain[4];
    hf::fr_from_mont(mont.l, plain);
    for (int i = 0; i < 32; i++) out[i] = (uint8_t)(plain[3 - i / 8] >> (8 * (7 - i % 8)));
}
// 32 big-endian bytes -> the plain integer's limbs
hf::Fr proof_be_limbs(const uint8_t in[32]) {
    hf::Fr v;
    for (int w = 0; w < 4; w++) {
        uint64_t x = 0;
        for (int b = 0; b < 8; b++) x = (x << 8) | in[24 - 8 * w + b];
        v.l[w] = x;
    }
    return v;
}
// a canonical scalar of the proof -> blst_fr; false when it is not below r
bool proof_fr_from_be(const uint8_t in[32], hf::Fr* out) {
    const hf::Fr v = proof_be_limbs(in);
    if (hf::fr_geq(v, hf::kFrMod)) return false;
    *out = hf::fr_mul(v, kFrR2);
    return true;
}
// fr(SHA256(state | tag)): the digest as a big-endian integer, reduced below r (2^256 < 3 r: at most two subtractions)
hf::Fr proof_challenge(const uint8_t state[32], uint8_t tag) {
    hf::Sha256 s;
    uint8_t d[32];
    hf::sha256_init(s);
    hf::sha256_update(s, state, 32);
    hf::sha256_update(s, &tag, 1);
    hf::sha256_final(s, d);
    hf::Fr v = proof_be_limbs(d);
    uint64_t br = 0;
    while (hf::fr_geq(v, hf::kFrMod)) v = hf::fr_raw_sub(v, hf::kFrMod, br);
    return hf::fr_mul(v, kFrR2);
}
// state <- SHA256(state | data)
void proof_absorb(uint8_t state[32], const uint8_t* data, size_t len) {
    hf::Sha256 s;
    hf::sha256_init(s);
    hf::sha256_update(s, state, 32);
    hf::sha256_update(s, data, len);
    hf::sha256_final(s, state);
}

enum ProofKind { kProofPlain, kProofCustom, kProofNext, kProofLookup };
// a run of the proof's bytes that the transcript absorbs whole, and the challenges drawn after it
struct ProofSegment {
    size_t off, len, draws;
};
constexpr size_t kProofMaxSegments = 6;  // a lookup proof's; no proof has more challenges than segments

// One proof format: everything the statement, the layout and the shape rules depend on.  shape_ok (or size_ok and lay_out, for a
// caller that has rho and no exponents) comes before anything that reads seg, nseg or len
struct ProofSpec {
    ProofKind kind;
    size_t n, t;
    unsigned log_ext;
    size_t n_public;
    size_t g = 0;  // the custom kinds: g terms, their g x t exponents, a next-row proof's second matrix
    const uint8_t *exps = nullptr, *exps_next = nullptr;
    size_t c = 0;    // the lookup kind: the table's columns
    size_t rho = 0;  // a next-row proof's wires with a next-row exponent (shape_ok counts them)
    ProofSegment seg[kProofMaxSegments] = {};
    size_t nseg = 0, len = 0;

    bool lookup() const { return kind == kProofLookup; }
    bool custom() const { return kind == kProofCustom || kind == kProofNext; }
    size_t nkey() const { return lookup() ? 2 * t + c + 3 : 2 * t + 2 + g; }
    size_t nevals() const { return lookup() ? 2 * t + c + 2 : 2 * t + rho; }
    size_t evals_off() const { return seg[nseg - 2].off; }
    size_t w_off() const { return seg[nseg - 1].off; }
    size_t npoints() const { return evals_off() / 48; }  // the points in front of the evaluations, at 48 i

    void lay_out() {
        const size_t e = (size_t)1 << log_ext;
        len = nseg = 0;
        auto add = [&](size_t bytes, size_t draws) {
            seg[nseg++] = ProofSegment{len, bytes, draws};
            len += bytes;
        };
        add(48 * t, lookup() ? 1 : 2);    // the wires, then theta, or beta and gamma
        if (lookup()) add(48, 2);         // [m], then beta and gamma
        add(lookup() ? 96 : 48, 1);       // [z] (and [phi]), then alpha
        add(48 * (e - 1), 1);             // T's chunks, then zeta
        add(32 * nevals(), 1);            // the evaluations, then v
        add(48, 0);                       // W
    }
    // the rules a proof's size depends on: t, log_ext and c or rho
    bool size_ok() const {
        if (t < KZG_CIRCUIT_MIN_COLUMNS || t > kPqMaxColumns || log_ext > kPqMaxLogExt) return false;
        const size_t e = (size_t)1 << log_ext;
        if (lookup()) return lookup_shape_ok(t, e, c);
        return t + 1 <= e && (kind != kProofNext || (rho >= 1 && rho <= t));
    }
    // the rules of every kind: n, t, log_ext and n_public as kzg_circuit_verify_proof takes them
    bool base_ok() const {
        PqShape sh;
        return log_ext <= kPqMaxLogExt && pq_shape(n, (size_t)1 << log_ext, &sh) && t >= KZG_CIRCUIT_MIN_COLUMNS && t <= kPqMaxColumns &&
               t + 1 <= sh.rot && n_public <= n;
    }
    // ... and the kind's own; counts rho and lays the proof out
    bool shape_ok() {
        if (!base_ok()) return false;
        const size_t e = (size_t)1 << log_ext;
        if (kind == kProofCustom && !custom_shape_ok(t, e, g, exps, nullptr)) return false;
        if (kind == kProofNext) rho = next_shape_rho(n, t, e, g, exps, exps_next, nullptr, nullptr);
        if (!size_ok()) return false;
        lay_out();
        return true;
    }

    // The statement in two halves.  The first: everything in front of the public inputs, into a fresh state (shifts: blst_fr images
    // below r)
    void statement_prefix(hf::Sha256& s, const uint64_t* key_p1s, const uint64_t* shifts) const {
        static const char* const kDst[] = {kProofDst, kCustomProofDst, kNextProofDst, kLookupProofDst};  // by ProofKind
        const char* dst = kDst[kind];
        uint8_t b[48];
        hf::sha256_init(s);
        hf::sha256_update(s, (const uint8_t*)dst, std::strlen(dst));
        const uint64_t header[5] = {n, t, log_ext, lookup() ? c : g, n_public};
        for (size_t i = 0; i < 5; i++) {
            if (i == 3 && kind == kProofPlain) continue;  // four words: neither g nor c
            for (int k = 0; k < 8; k++) b[k] = (uint8_t)(header[i] >> (8 * (7 - k)));
            hf::sha256_update(s, b, 8);
        }
        for (size_t j = 0; j < t; j++) {
            proof_fr_to_be(pq_fr(shifts + 4 * j), b);
            hf::sha256_update(s, b, 32);
        }
        if (custom()) hf::sha256_update(s, exps, g * t);
        if (kind == kProofNext) hf::sha256_update(s, exps_next, g * t);
        for (size_t j = 0; j < nkey(); j++) {
            hf::P1 k;
            std::memcpy(&k, key_p1s + 18 * j, sizeof k);
            hf::p1_compress(b, k);
            hf::sha256_update(s, b, 48);
        }
    }
    // The second: the public inputs (blst_fr images below r) in one pass, through a block on the stack; h0.  The state is spent
    void statement_finish(hf::Sha256& s, const uint64_t* public_inputs, uint8_t h0[32]) const {
        uint8_t b[32 * 128];
        for (size_t i = 0; i < n_public; i += 128) {
            const size_t m = n_public - i < 128 ? n_public - i : 128;
            for (size_t k = 0; k < m; k++) proof_fr_to_be(pq_fr(public_inputs + 4 * (i + k)), b + 32 * k);
            hf::sha256_update(s, b, 32 * m);
        }
        hf::sha256_final(s, h0);
    }
};

// The walk over a proof's rounds: h holds h_i; round() absorbs segment i and draws its challenges behind those drawn so far, so ch
// fills in the order the *_proof_challenges calls give them: (theta,) beta, gamma, alpha, zeta, v.  The prover calls round() as each
// segment of its proof becomes known, run() takes complete bytes
struct ProofWalk {
    uint8_t h[32];
    size_t next = 0, drawn = 0;
    hf::Fr ch[kProofMaxSegments];
    void round(const ProofSpec& sp, const uint8_t* proof) {
        const ProofSegment& sg = sp.seg[next++];
        proof_absorb(h, proof + sg.off, sg.len);
        for (size_t d = 0; d < sg.draws; d++) ch[drawn++] = proof_challenge(h, (uint8_t)d);
    }
    // stmt: the statement's prefix absorbed (a copy: a batch shares one); every segment in front of W
    void run(const ProofSpec& sp, hf::Sha256 stmt, const uint64_t* public_inputs, const uint8_t* proof) {
        sp.statement_finish(stmt, public_inputs, h);
        while (next + 1 < sp.nseg) round(sp, proof);
    }
};
// the shifts and the public inputs are blst_fr images below r
static bool proof_scalars_ok(const uint64_t* shifts, size_t t, const uint64_t* public_inputs, size_t n_public) {
    hf::Fr v;
    for (size_t j = 0; j < t; j++)
        if (!fr_arg_below_r(shifts + 4 * j, &v)) return false;
    for (size_t i = 0; i < n_public; i++)
        if (!fr_arg_below_r(public_inputs + 4 * i, &v)) return false;
    return true;
}
// What every host call on proof bytes refuses with KZG_ERR_INVALID_ARG: a null argument, a shape that is not the kind's, a proof_len
// that is not the format's, a shift or a public input not below r.  Lays sp out
static bool proof_call_ok(ProofSpec& sp, const uint64_t* key_p1s, const uint64_t* shifts, const uint64_t* public_inputs,
                          const uint8_t* proof, size_t proof_len) {
    if (!key_p1s || !shifts || (!public_inputs && sp.n_public) || !proof) return false;
    if ((sp.custom() && !sp.exps) || (sp.kind == kProofNext && !sp.exps_next)) return false;
    return sp.shape_ok() && proof_len == sp.len && proof_scalars_ok(shifts, sp.t, public_inputs, sp.n_public);
}
// the *_proof_size calls (sp: t, log_ext and c or rho)
static int proof_size_impl(ProofSpec sp, size_t* bytes) {
    if (!bytes || !sp.size_ok()) return KZG_ERR_INVALID_ARG;
    sp.lay_out();
    *bytes = sp.len;
    return KZG_OK;
}
// the *_proof_challenges calls: out receives 4 u64 a challenge, in ProofWalk's order
static int proof_challenges_impl(ProofSpec sp, const uint64_t* key_p1s, const uint64_t* shifts, const uint64_t* public_inputs,
                                 const uint8_t* proof, size_t proof_len, uint64_t* out) {
    if (!out || !proof_call_ok(sp, key_p1s, shifts, public_inputs, proof, proof_len)) return KZG_ERR_INVALID_ARG;
    hf::Sha256 stmt;
    sp.statement_prefix(stmt, key_p1s, shifts);
    ProofWalk w;
    w.run(sp, stmt, public_inputs, proof);
    for (size_t i = 0; i < w.drawn; i++) std::memcpy(out + 4 * i, w.ch[i].l, 32);
    return KZG_OK;
}
// the *_verify_proof calls: the checks, the key's commitments on the curve before the proof is looked at (kzg_circuit_verify's
// check), the proof's points (on the curve; no subgroup check) and canonical scalars -- a proof that does not decode is invalid, not
// an error -- the challenges, and the kind's claim to circuit_verify_impl
int verify_proof_impl(ProofSpec sp, const uint64_t* key_p1s, const uint64_t* shifts, const uint64_t* public_inputs, const uint8_t* proof,
                      size_t proof_len, const void* setup_g1, size_t g1_stride_bytes, const void* setup_g2, size_t g2_stride_bytes,
                      int* valid) {
    if (!setup_g1 || !setup_g2 || !valid || !proof_call_ok(sp, key_p1s, shifts, public_inputs, proof, proof_len)) return KZG_ERR_INVALID_ARG;
    for (size_t j = 0; j < sp.nkey(); j++) {
        hf::P1 k;
        std::memcpy(&k, key_p1s + 18 * j, sizeof k);
        if (!hf::p1_on_curve(k)) return KZG_ERR_INVALID_ARG;
    }
    const size_t t = sp.t, npts = sp.npoints(), nlk = sp.lookup() ? 1 : 0;
    std::vector<uint64_t> pts(18 * npts), evals(4 * sp.nevals());
    uint64_t w_p1[18];
    bool decoded = true;
    for (size_t i = 0; i < npts && decoded; i++) decoded = kzg_g1_uncompress(proof + 48 * i, pts.data() + 18 * i) == KZG_OK;
    decoded = decoded && kzg_g1_uncompress(proof + sp.w_off(), w_p1) == KZG_OK;
    for (size_t i = 0; i < sp.nevals() && decoded; i++) {
        hf::Fr v = kFrZero;
        decoded = proof_fr_from_be(proof + sp.evals_off() + 32 * i, &v);
        std::memcpy(evals.data() + 4 * i, v.l, 32);
    }
    if (!decoded) {
        *valid = 0;
        return KZG_OK;
    }
    hf::Sha256 stmt;
    sp.statement_prefix(stmt, key_p1s, shifts);
    ProofWalk w;
    w.run(sp, stmt, public_inputs, proof);
    // the points: wires, ([m],) [z], ([phi],) chunks; the challenges behind a lookup proof's theta: beta, gamma, alpha, zeta, v
    const uint64_t *z_p1 = pts.data() + 18 * (t + nlk), *t_p1s = pts.data() + 18 * (t + 1 + 2 * nlk);
    const hf::Fr* ch = w.ch + nlk;
    const LookupClaim lookup{sp.c, w.ch[0].l, pts.data() + 18 * t, pts.data() + 18 * (t + 2)};
    const CustomClaim custom{sp.g, sp.exps, sp.exps_next, sp.kind == kProofNext ? evals.data() + 4 * 2 * t : nullptr};
    return circuit_verify_impl(key_p1s, sp.n, t, sp.log_ext, shifts, pts.data(), z_p1, t_p1s, public_inputs, sp.n_public, evals.data(),
                               ch[2].l, ch[0].l, ch[1].l, ch[3].l, ch[4].l, w_p1, setup_g1, g1_stride_bytes, setup_g2, g2_stride_bytes, valid,
                               nlk ? &lookup : nullptr, sp.custom() ? &custom : nullptr);
}
}  // namespace

int kzg_circuit_proof_size(size_t t, unsigned log_ext, size_t* bytes) {
    return proof_size_impl(ProofSpec{kProofPlain, 0, t, log_ext, 0}, bytes);
}

int kzg_circuit_custom_next_proof_size(size_t t, unsigned log_ext, size_t rho, size_t* bytes) {
    ProofSpec sp{kProofNext, 0, t, log_ext, 0};
    sp.rho = rho;
    return proof_size_impl(sp, bytes);
}

int kzg_circuit_lookup_proof_size(size_t t, unsigned log_ext, size_t c, size_t* bytes) {
    return proof_size_impl(ProofSpec{kProofLookup, 0, t, log_ext, 0, 0, nullptr, nullptr, c}, bytes);
}

int kzg_circuit_proof_challenges(const uint64_t* key_p1s, size_t n, size_t t, unsigned log_ext, const uint64_t* shifts,
                                 const uint64_t* public_inputs, size_t n_public, const uint8_t* proof, size_t proof_len, uint64_t* out) {
    return proof_challenges_impl(ProofSpec{kProofPlain, n, t, log_ext, n_public}, key_p1s, shifts, public_inputs, proof, proof_len, out);
}

int kzg_circuit_custom_proof_challenges(const uint64_t* key_p1s, size_t n, size_t t, unsigned log_ext, size_t g, const uint8_t* exponents,
                                        const uint64_t* shifts, const uint64_t* public_inputs, size_t n_public, const uint8_t* proof,
                                        size_t proof_len, uint64_t* out) {
    return proof_challenges_impl(ProofSpec{kProofCustom, n, t, log_ext, n_public, g, exponents}, key_p1s, shifts, public_inputs, proof,
                                 proof_len, out);
}

int kzg_circuit_custom_next_proof_challenges(const uint64_t* key_p1s, size_t n, size_t t, unsigned log_ext, size_t g,
                                             const uint8_t* exponents, const uint8_t* exponents_next, const uint64_t* shifts,
                                             const uint64_t* public_inputs, size_t n_public, const uint8_t* proof, size_t proof_len,
                                             uint64_t* out) {
    return proof_challenges_impl(ProofSpec{kProofNext, n, t, log_ext, n_public, g, exponents, exponents_next}, key_p1s, shifts,
                                 public_inputs, proof, proof_len, out);
}

int kzg_circuit_lookup_proof_challenges(const uint64_t* key_p1s, size_t n, size_t t, unsigned log_ext, size_t c, const uint64_t* shifts,
                                        const uint64_t* public_inputs, size_t n_public, const uint8_t* proof, size_t proof_len,
                                        uint64_t* out) {
    return proof_challenges_impl(ProofSpec{kProofLookup, n, t, log_ext, n_public, 0, nullptr, nullptr, c}, key_p1s, shifts, public_inputs,
                                 proof, proof_len, out);
}

int kzg_circuit_verify_proof(const uint64_t* key_p1s, size_t n, size_t t, unsigned log_ext, const uint64_t* shifts,
                             const uint64_t* public_inputs, size_t n_public, const uint8_t* proof, size_t proof_len, const void* setup_g1,
                             size_t g1_stride_bytes, const void* setup_g2, size_t g2_stride_bytes, int* valid) {
    return verify_proof_impl(ProofSpec{kProofPlain, n, t, log_ext, n_public}, key_p1s, shifts, public_inputs, proof, proof_len, setup_g1,
                             g1_stride_bytes, setup_g2, g2_stride_bytes, valid);
}

int kzg_circuit_custom_verify_proof(const uint64_t* key_p1s, size_t n, size_t t, unsigned log_ext, size_t g, const uint8_t* exponents,
                                    const uint64_t* shifts, const uint64_t* public_inputs, size_t n_public, const uint8_t* proof,
                                    size_t proof_len, const void* setup_g1, size_t g1_stride_bytes, const void* setup_g2,
                                    size_t g2_stride_bytes, int* valid) {
    return verify_proof_impl(ProofSpec{kProofCustom, n, t, log_ext, n_public, g, exponents}, key_p1s, shifts, public_inputs, proof,
                             proof_len, setup_g1, g1_stride_bytes, setup_g2, g2_stride_bytes, valid);
}

int kzg_circuit_custom_next_verify_proof(const uint64_t* key_p1s, size_t n, size_t t, unsigned log_ext, size_t g, const uint8_t* exponents,
                                         const uint8_t* exponents_next, const uint64_t* shifts, const uint64_t* public_inputs,
                                         size_t n_public, const uint8_t* proof, size_t proof_len, const void* setup_g1,
                                         size_t g1_stride_bytes, const void* setup_g2, size_t g2_stride_bytes, int* valid) {
    return verify_proof_impl(ProofSpec{kProofNext, n, t, log_ext, n_public, g, exponents, exponents_next}, key_p1s, shifts, public_inputs,
                             proof, proof_len, setup_g1, g1_stride_bytes, setup_g2, g2_stride_bytes, valid);
}

int kzg_circuit_lookup_verify_proof(const uint64_t* key_p1s, size_t n, size_t t, unsigned log_ext, size_t c, const uint64_t* shifts,
                                    const uint64_t* public_inputs, size_t n_public, const uint8_t* proof, size_t proof_len,
                                    const void* setup_g1, size_t g1_stride_bytes, const void* setup_g2, size_t g2_stride_bytes,
                                    int* valid) {
    return verify_proof_impl(ProofSpec{kProofLookup, n, t, log_ext, n_public, 0, nullptr, nullptr, c}, key_p1s, shifts, public_inputs,
                             proof, proof_len, setup_g1, g1_stride_bytes, setup_g2, g2_stride_bytes, valid);
}

// ---- many proofs of one key with one pairing check (circuit_verify_kernels.hip) ----------------------------
// The host hashes the transcripts (up to 16 threads), draws the weights and pairs P0, P1, P2 once; the device decodes the points and
// the evaluations, computes PI(zeta_k) and every scalar of the identity, checks the points to lie in G1, runs every scalar
// multiplication and the sums.
namespace {
int circuit_verify_batch_impl(kzg_ctx* ctx, const uint64_t* key_p1s, size_t n, size_t t, unsigned log_ext, size_t g, const uint8_t* exps,
                              const uint64_t* shifts, const uint64_t* public_inputs, size_t n_public, size_t pi_stride,
                              const uint8_t* proofs, size_t proof_len, size_t count, const void* setup_g2, size_t g2_stride_bytes,
                              const uint64_t* weights, bool want_weights, uint64_t* out_p1s, int* valid, size_t* bad_index,
                              const uint64_t* challenges = nullptr) {
    if (!ctx) return KZG_ERR_INVALID_ARG;
    const char* what = "circuit verify batch";
    auto invalid = [&](const std::string& why) {
        ctx->last_error = std::string(what) + ": " + why;
        return KZG_ERR_INVALID_ARG;
    };
    if (!key_p1s || !shifts || (!public_inputs && n_public && count) || (!proofs && count) || !setup_g2 || !valid ||
        (want_weights && (!out_p1s || (!weights && count))) || (g && !exps))
        return invalid("a required pointer is NULL");
    ProofSpec sp{exps ? kProofCustom : kProofPlain, n, t, log_ext, n_public, g, exps};
    if (!sp.base_ok()) return invalid("n, t, log_ext or n_public is not a shape of kzg_circuit_verify_proof");
    if (!sp.shape_ok()) return invalid("g or the exponents are not a shape of the custom verifier");
    const size_t e = (size_t)1 << log_ext;
    if (proof_len != sp.len) return invalid("proof_len is not kzg_circuit_proof_size's");
    if (count > KZG_VERIFY_MAX_PROOFS) return invalid("more than KZG_VERIFY_MAX_PROOFS proofs");
    if (n < 2) return invalid("n < 2: the two point sets of a proof coincide");
    if (pi_stride < n_public && count > 1) return invalid("pi_stride is below n_public");
    if (!proof_scalars_ok(shifts, t, nullptr, 0)) return invalid("a shift is not below r");
    for (size_t k = 0; k < count; k++)  // validated here, converted again by the thread that hashes proof k: nothing of size count is kept
        for (size_t i = 0; i < n_public; i++) {
            hf::Fr v;
            if (!fr_arg_below_r(public_inputs + 4 * (k * pi_stride + i), &v))
                return invalid("proof " + std::to_string(k) + ": public input " + std::to_string(i) + " is not below r");
        }
    const size_t nkey = sp.nkey(), nk = nkey + 1;  // the key's commitments, then G1
    for (size_t j = 0; j < nkey; j++) {
        hf::P1 c;
        std::memcpy(&c, key_p1s + 18 * j, sizeof c);
        if (!hf::p1_on_curve(c)) return invalid("key commitment " + std::to_string(j) + " is not on the curve");
    }
    hf::G2Affine g2[3];
    for (int i = 0; i < 3; i++) {
        uint64_t raw[36];
        std::memcpy(raw, (const uint8_t*)setup_g2 + i * g2_stride_bytes, sizeof raw);
        g2[i] = hf::g2_from_p2(raw);
        if (!hf::g2_on_curve(g2[i])) return invalid("setup_g2[" + std::to_string(i) + "] is not on the twist");
    }
    if (want_weights)
        for (size_t k = 0; k < count; k++) {
            hf::Fr w;
            std::memcpy(w.l, weights + 4 * k, 32);
            if (hf::fr_geq(w, hf::kFrMod)) return invalid("weight " + std::to_string(k) + " is not below r");
        }
    for (size_t i = 0; challenges && i < 5 * count; i++) {
        hf::Fr c;
        std::memcpy(c.l, challenges + 4 * i, 32);
        if (hf::fr_geq(c, hf::kFrMod)) return invalid("proof " + std::to_string(i / 5) + ": a challenge is not below r");
    }
    if (bad_index) *bad_index = (size_t)-1;
    if (!count) {
        if (want_weights) {
            const hf::P1 inf = hf::p1_inf();
            for (int i = 0; i < 3; i++) write_p1(out_p1s + 18 * i, inf);
        }
        *valid = 1;
        return KZG_OK;
    }
    if (ctx->multi) {
        kzg_ctx* kid = whole_srs_kid(ctx, true, "circuit verify batch needs");
        if (!kid) return KZG_ERR_INVALID_ARG;
        return forwarded(ctx, kid, circuit_verify_batch_impl(kid, key_p1s, n, t, log_ext, g, exps, shifts, public_inputs, n_public, pi_stride,
                                                             proofs, proof_len, count, setup_g2, g2_stride_bytes, weights, want_weights,
                                                             out_p1s, valid, bad_index, challenges));
    }
    PqShape sh;
    pq_shape(n, e, &sh);
    const size_t M = count, R = t + e + 1;  // a proof's points: t wires, [z], e - 1 chunks, W
    std::vector<hf::Fr> rho;
    std::vector<Glv> rho_glv;
    {
        const int rcw = vc_weights(ctx, what, want_weights ? weights : nullptr, M, &rho, &rho_glv);
        if (rcw) return rcw;
    }
    // the statement's bytes in front of the public inputs, hashed once
    hf::Sha256 stmt;
    sp.statement_prefix(stmt, key_p1s, shifts);
    // lanes of the one ladder launch: [the R - 1 points of A_0 per proof | W per proof | the key's nk points with their scalars of P0 |
    // the same with those of P1 | [z] per proof, a second time].  Affine records: the key's nk in front, so that the least failing
    // index names a key commitment (an error) before any proof (a verdict), then the proofs' NP
    const size_t NP = M * R, lanes = M * (R + 1) + 2 * nk, oF = M * (R - 1), oK = oF + M, oE = oK + 2 * nk;
    // the host's part: the five challenges of every proof (ProofWalk over each proof's bytes), as blst_fr images
    std::vector<uint64_t> chal(20 * M);
    std::vector<uint32_t> src(lanes);
    size_t nthreads = std::min<size_t>({(size_t)16, std::max<size_t>(1, std::thread::hardware_concurrency()), M});
    auto work = [&](size_t th) {
        for (size_t k = th; k < M; k += nthreads) {
            const uint8_t* proof = proofs + k * proof_len;
            for (size_t i = 0; i + 1 < R; i++) src[k * (R - 1) + i] = (uint32_t)(nk + k * R + i);
            src[oF + k] = (uint32_t)(nk + k * R + R - 1);
            src[oE + k] = (uint32_t)(nk + k * R + t);
            if (challenges) {  // the test hook's: nothing is hashed
                std::memcpy(&chal[20 * k], challenges + 20 * k, 160);
                continue;
            }
            ProofWalk w;  // from a copy of the prefix's state
            w.run(sp, stmt, n_public ? public_inputs + 4 * k * pi_stride : nullptr, proof);
            // the kernels' order: beta, gamma, alpha, zeta, v
            for (int i = 0; i < 5; i++) std::memcpy(&chal[20 * k + 4 * i], w.ch[i].l, 32);
        }
    };
    if (nthreads <= 1) {
        work(0);
    } else {
        std::vector<std::thread> pool;
        for (size_t th = 1; th < nthreads; th++) pool.emplace_back(work, th);
        work(0);
        for (auto& th : pool) th.join();
    }
    for (size_t j = 0; j < 2 * nk; j++) src[oK + j] = (uint32_t)(j % nk);
    // the kernels' constants, multiplier form: 2^14, w, 1 + w, 1 / n, w^64, the shifts
    std::vector<Fr30> consts(kCvbShifts + t);
    {
        const hf::Fr w = hf::fr_domain_root(sh.lg_n);
        consts[kCvbK284] = fr30_arg_from_mont256(fr_pow2(14));
        consts[kCvbW] = fr30_arg_from_mont256(w);
        consts[kCvbW1] = fr30_arg_from_mont256(hf::fr_add(w, hf::kFrOne));
        consts[kCvbInvN] = fr30_arg_from_mont256(hf::fr_inv(fr_pow2(sh.lg_n)));
        consts[kCvbW64] = fr30_arg_from_mont256(hf::fr_pow(w, 64));
        for (size_t j = 0; j < t; j++) consts[kCvbShifts + j] = fr30_arg_from_mont256(pq_fr(shifts + 4 * j));
    }
    // XYZZ records, laid out so that every side is a run of consecutive records:
    //   [the ladder's products of A_0: M (R - 1) | F: M | P0's terms: 3 M | the key's for P0: nk | the key's for P1: nk | E: M | D: M |
    //    [zeta (1 + w)] F: M | the three sums]
    // P2' = sum F, P0 and P1 are three consecutive segments from F on; D_k is the sum of proof k's R - 1 products
    const size_t oP0 = M * R, oKey = oP0 + 3 * M, oEr = oKey + 2 * nk, oD = oEr + M, oS3 = oD + M, oOut = oS3 + M;
    // the key side's rows: 2 nk values a proof, padded to a power of two, summed over the proofs
    uint32_t log_l = 0;
    while (((size_t)1 << log_l) < 2 * nk) log_l++;
    const size_t l = (size_t)1 << log_l;
    VcPlan plan_d, plan_fin, plan_rows;
    vc_plan(std::vector<uint32_t>(M, (uint32_t)(R - 1)), &plan_d);
    vc_plan({(uint32_t)M, (uint32_t)(3 * M + nk), (uint32_t)(nk + 3 * M)}, &plan_fin);
    vc_plan({(uint32_t)M}, &plan_rows);
    std::vector<uint32_t> starts;
    std::vector<size_t> at_d, at_fin, at_rows;
    for (auto* pl : {&plan_d, &plan_fin, &plan_rows}) {
        auto& at = pl == &plan_d ? at_d : (pl == &plan_fin ? at_fin : at_rows);
        for (const auto& lv : *pl) {
            at.push_back(starts.size());
            starts.insert(starts.end(), lv.begin(), lv.end());
        }
    }
    const size_t gmax = std::max(plan_d[0].size() - 1, plan_fin[0].size() - 1), grows = plan_rows[0].size() - 1;
    const size_t pub_values = n_public ? (M - 1) * pi_stride + n_public : 0;  // as the caller laid them out
    std::lock_guard<std::mutex> lkf(ctx->fk20_mu);  // guards the workspaces
    std::unique_lock<std::mutex> lk(ctx->mu);
    if (!ctx->n || !ctx->slots_ready) {
        ctx->last_error = std::string(what) + ": the SRS is empty";
        return KZG_ERR_NO_SRS;
    }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const int slot = reserve_slot(ctx, lk, true);
    if (slot < 0) return KZG_ERR_BUSY;
    SlotLease lease{ctx, slot};
    Slot& s = ctx->slots[slot];
    int rc = ensure_slot_basics(ctx, s);
    void *wire = nullptr, *coef = nullptr, *dstarts = nullptr, *p1 = nullptr, *aff = nullptr, *prefix = nullptr, *dsrc = nullptr,
         *dglv = nullptr, *dglvs = nullptr, *g1 = nullptr, *scratch = nullptr, *cells = nullptr, *fa = nullptr, *fb = nullptr, *frs = nullptr,
         *dpub = nullptr;
    // the Fr inputs behind one another in one workspace: evaluations' bytes | their images | challenges | weights | PI(zeta) | consts |
    // exponents | k_cvb_lin's records (each part a multiple of 32 bytes)
    const size_t fEvB = 0, fEv = fEvB + M * 64 * t, fCh = fEv + M * 64 * t, fRho = fCh + M * 160, fPi = fRho + M * 32,
                 fCo = fPi + ((M * sizeof(Fr30) + 31) / 32) * 32, fEx = fCo + ((consts.size() * sizeof(Fr30) + 31) / 32) * 32,
                 fLin = fEx + ((g * t + 31) / 32) * 32, fEnd = fLin + 4 * M * sizeof(Fr30);
    if (rc == KZG_OK) rc = ctx->vc_ws.get(ctx, kVcWire, NP * 48, &wire);
    if (rc == KZG_OK) rc = ctx->vc_ws.get(ctx, kVcCoefA, kVcErrWords * 4, &coef);
    if (rc == KZG_OK) rc = ctx->vc_ws.get(ctx, kVcStarts, starts.size() * 4, &dstarts);
    if (rc == KZG_OK) rc = ctx->vc_ws.get(ctx, kVcP1, nk * 144, &p1);
    if (rc == KZG_OK) rc = ctx->vc_ws.get(ctx, kVcAff, (NP + nk) * kAffineBytes, &aff);
    if (rc == KZG_OK) rc = ctx->vc_ws.get(ctx, kVcPrefix, nk * 64, &prefix);
    if (rc == KZG_OK) rc = ctx->vc_ws.get(ctx, kVcSrc, lanes * 4, &dsrc);
    if (rc == KZG_OK) rc = ctx->vc_ws.get(ctx, kVcGlv, lanes * sizeof(Glv), &dglv);
    if (rc == KZG_OK) rc = ctx->vc_ws.get(ctx, kVcGlvSrs, 4 * M * sizeof(Glv), &dglvs);
    if (rc == KZG_OK) rc = ctx->vc_ws.get(ctx, kVcG1, (oOut + 3) * kXyzzBytes, &g1);
    if (rc == KZG_OK) rc = ctx->vc_ws.get(ctx, kVcScratch, 2 * gmax * kXyzzBytes, &scratch);
    if (rc == KZG_OK) rc = ctx->vc_ws.get(ctx, kVcCells, M * l * 32, &cells);
    if (rc == KZG_OK) rc = ctx->vc_ws.get(ctx, kVcFrA, grows * l * 32, &fa);
    if (rc == KZG_OK) rc = ctx->vc_ws.get(ctx, kVcFrB, grows * l * 32, &fb);
    if (rc == KZG_OK) rc = ctx->vc_ws.get(ctx, kVcRho, fEnd, &frs);
    if (rc == KZG_OK && pub_values) rc = ctx->vc_ws.get(ctx, kVcOrder, pub_values * 32, &dpub);
    if (rc) return rc;
    const hipStream_t st = s.stream;
    uint32_t* err = (uint32_t*)coef;  // the ladder's words at kVcErrCurve / kVcErrG1, the decoders' at kVcErrWireProof / kVcErrWireValue
    Glv* ds2 = (Glv*)dglvs;
    void* proof_aff = (char*)aff + nk * kAffineBytes;
    auto rec = [&](size_t i) { return (void*)((char*)g1 + i * kXyzzBytes); };
    auto fr_at = [&](size_t off) { return (uint32_t*)((char*)frs + off); };
    HIP_TRY(ctx, hipMemsetAsync(err, 0xff, kVcErrWords * 4, st));
    // the proofs' bytes as received: the points (the wires, [z] and the chunks, then W) and the evaluations, each field of a proof
    // to its place by a strided copy
    HIP_TRY(ctx, hipMemcpy2DAsync(wire, 48 * R, proofs, proof_len, 48 * (R - 1), M, hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipMemcpy2DAsync((char*)wire + 48 * (R - 1), 48 * R, proofs + sp.w_off(), proof_len, 48, M, hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipMemcpy2DAsync(fr_at(fEvB), 64 * t, proofs + sp.evals_off(), proof_len, 64 * t, M, hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipMemcpyAsync(fr_at(fCh), chal.data(), M * 160, hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipMemcpyAsync(fr_at(fRho), rho.data(), M * 32, hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipMemcpyAsync(fr_at(fCo), consts.data(), consts.size() * sizeof(Fr30), hipMemcpyHostToDevice, st));
    if (g) HIP_TRY(ctx, hipMemcpyAsync(fr_at(fEx), exps, g * t, hipMemcpyHostToDevice, st));
    if (pub_values) HIP_TRY(ctx, hipMemcpyAsync(dpub, public_inputs, pub_values * 32, hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipMemcpyAsync(dstarts, starts.data(), starts.size() * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipMemcpyAsync(dsrc, src.data(), lanes * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipMemcpyAsync((Glv*)dglv + oF, rho_glv.data(), M * sizeof(Glv), hipMemcpyHostToDevice, st));  // F_k = [rho_k] W_k
    HIP_TRY(ctx, hipMemsetAsync(cells, 0, M * l * 32, st));
    // the key's records, then G1 = SRS[0] from the table's level 0; the proofs' points decoded behind them
    HIP_TRY(ctx, hipMemcpyAsync(p1, key_p1s, nkey * 144, hipMemcpyHostToDevice, st));
    launch_jacobian_to_affine(st, p1, (uint32_t)nkey, aff, prefix);
    HIP_TRY(ctx, hipMemcpyAsync((char*)aff + nkey * kAffineBytes, ctx->table.p, kAffineBytes, hipMemcpyDeviceToDevice, st));
    launch_wire_g1(st, wire, nullptr, (uint32_t)NP, proof_aff, (uint32_t)kAffineBytes, err + kVcErrWireProof);
    // the Fr side: the evaluations decoded, PI(zeta_k), every proof's scalars split for the ladders and its row of key-side terms,
    // the rows summed over the proofs, the sums split
    launch_wire_fr(st, fr_at(fEvB), (uint32_t)(M * 2 * t), 0, false, fr_at(fEv), err + kVcErrWireValue);
    const Fr30* dconsts = (const Fr30*)fr_at(fCo);
    if (n_public)
        launch_cvb_public(st, (const uint32_t*)dpub, (uint32_t)n_public, pi_stride, fr_at(fCh), dconsts, sh.lg_n, (uint32_t)M, (Fr30*)fr_at(fPi));
    launch_cvb_scalars(st, fr_at(fCh), fr_at(fEv), fr_at(fRho), n_public ? (const Fr30*)fr_at(fPi) : nullptr, dconsts,
                       g ? (const uint8_t*)fr_at(fEx) : nullptr, (uint32_t)M, (uint32_t)t, (uint32_t)e, (uint32_t)g, sh.lg_n, (Fr30*)fr_at(fLin), (Glv*)dglv, oE,
                       ds2, (uint32_t*)cells, log_l);
    const uint32_t* dst_ = (const uint32_t*)dstarts;
    const uint32_t* key_sums = (const uint32_t*)cells;
    for (size_t lv = 0; lv < plan_rows.size(); lv++) {
        uint32_t* dst = key_sums == (uint32_t*)fa ? (uint32_t*)fb : (uint32_t*)fa;
        launch_vc_fr_sum(st, key_sums, nullptr, nullptr, dst_ + at_rows[lv], (uint32_t)(plan_rows[lv].size() - 1), log_l, dst);
        key_sums = dst;
    }
    launch_cvb_key_split(st, key_sums, (uint32_t)(2 * nk), (Glv*)dglv + oK);
    // stage 1: every point times its scalar in one launch; the proofs' points and the key's commitments are checked (lanes below
    // M R + nkey: the key's second copy, G1 and the second [z] are not checked again)
    launch_vc_ladder(st, aff, (const uint32_t*)dsrc, (const Glv*)dglv, (uint32_t)lanes, (uint32_t)(M * R + nkey), (uint32_t)(M * R), rec(0),
                     rec(oKey), err);
    void* X[2] = {scratch, (char*)scratch + gmax * kXyzzBytes};
    auto g1_plan = [&](const VcPlan& plan, const std::vector<size_t>& at, const void* in, void* out) {
        const void* c = in;
        for (size_t lv = 0; lv < plan.size(); lv++) {
            void* dst = lv + 1 == plan.size() ? out : (c == X[0] ? X[1] : X[0]);
            launch_vc_g1_sum(st, c, dst_ + at[lv], (uint32_t)(plan[lv].size() - 1), dst);
            c = dst;
        }
    };
    g1_plan(plan_d, at_d, rec(0), rec(oD));
    // stage 2: the proofs' products for P0 and P1; then the three sums P2' = sum F, P0, P1
    launch_cvb_stage2(st, rec(oD), rec(oEr), rec(oF), ds2, (uint32_t)M, rec(oP0), rec(oS3));
    g1_plan(plan_fin, at_fin, rec(oF), rec(oOut));
    launch_xyzz_to_affine(st, rec(oOut), 3, aff, prefix);
    launch_affine_to_p1(st, aff, 3, p1);
    HIP_TRY(ctx, hipGetLastError());
    uint32_t herr[kVcErrWords];
    uint64_t sides[54];
    HIP_TRY(ctx, hipMemcpyAsync(herr, err, sizeof herr, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipMemcpyAsync(sides, p1, sizeof sides, hipMemcpyDeviceToHost, st));
    rc = sync_unlocked(ctx, lk, st, what);
    if (rc) return rc;
    const uint32_t grp = std::min(herr[kVcErrCurve], herr[kVcErrG1]);  // a record index: the key's are below nk
    if (grp < nk) return invalid("key commitment " + std::to_string(grp) + " is not in G1");
    // a proof that does not decode (a point, an evaluation) or has a point outside G1 is invalid, not an error: the least such proof
    size_t bad = (size_t)-1;
    if (grp != 0xffffffffu) bad = (grp - nk) / R;
    if (herr[kVcErrWireProof] != 0xffffffffu) bad = std::min(bad, (size_t)herr[kVcErrWireProof] / R);
    if (herr[kVcErrWireValue] != 0xffffffffu) bad = std::min(bad, (size_t)herr[kVcErrWireValue] / (2 * t));
    if (bad != (size_t)-1) {
        if (bad_index) *bad_index = bad;
        if (want_weights) {
            const hf::P1 inf = hf::p1_inf();
            for (int i = 0; i < 3; i++) write_p1(out_p1s + 18 * i, inf);
        }
        *valid = 0;
        return KZG_OK;
    }
    hf::P1 sums[3], ps[3];  // the device's order: sum F, P0, P1
    std::memcpy(sums, sides, sizeof sides);
    ps[0] = sums[1];
    ps[1] = sums[2];
    ps[2] = hf::p1_neg(sums[0]);
    if (want_weights)
        for (int i = 0; i < 3; i++) write_p1(out_p1s + 18 * i, ps[i]);
    bool ok = true;
    const hf::F12 f = hf::multi_miller_loop(g2, ps, 3, ok);
    *valid = ok && hf::f12_is_one(hf::f12_final_exp(f)) ? 1 : 0;
    return KZG_OK;
}
}  // namespace

int kzg_circuit_verify_proofs_batch(kzg_ctx* ctx, const uint64_t* key_p1s, size_t n, size_t t, unsigned log_ext, size_t g,
                                    const uint8_t* exponents, const uint64_t* shifts, const uint64_t* public_inputs, size_t n_public,
                                    size_t pi_stride, const uint8_t* proofs, size_t proof_len, size_t count, const void* setup_g2,
                                    size_t g2_stride_bytes, int* valid, size_t* bad_index) {
    try {
        return circuit_verify_batch_impl(ctx, key_p1s, n, t, log_ext, g, exponents, shifts, public_inputs, n_public, pi_stride, proofs,
                                         proof_len, count, setup_g2, g2_stride_bytes, nullptr, false, nullptr, valid, bad_index);
    } catch (...) {  // nothing may unwind through the C-ABI: the host vectors of a large batch, or a thread that could not start
        ctx->last_error = "circuit verify batch: out of host memory or threads";
        return KZG_ERR_HIP;
    }
}

int kzg_circuit_verify_proofs_lincomb_challenges(kzg_ctx* ctx, const uint64_t* key_p1s, size_t n, size_t t, unsigned log_ext, size_t g,
                                                 const uint8_t* exponents, const uint64_t* shifts, const uint64_t* public_inputs,
                                                 size_t n_public, size_t pi_stride, const uint8_t* proofs, size_t proof_len, size_t count,
                                                 const void* setup_g2, size_t g2_stride_bytes, const uint64_t* weights,
                                                 const uint64_t* challenges, uint64_t out_p1s[54], int* valid, size_t* bad_index) {
    if (ctx && count && !challenges) {
        ctx->last_error = "circuit verify batch: a required pointer is NULL";
        return KZG_ERR_INVALID_ARG;
    }
    try {
        return circuit_verify_batch_impl(ctx, key_p1s, n, t, log_ext, g, exponents, shifts, public_inputs, n_public, pi_stride, proofs,
                                         proof_len, count, setup_g2, g2_stride_bytes, weights, true, out_p1s, valid, bad_index, challenges);
    } catch (...) {
        ctx->last_error = "circuit verify batch: out of host memory or threads";
        return KZG_ERR_HIP;
    }
}

int kzg_circuit_verify_proofs_lincomb(kzg_ctx* ctx, const uint64_t* key_p1s, size_t n, size_t t, unsigned log_ext, size_t g,
                                      const uint8_t* exponents, const uint64_t* shifts, const uint64_t* public_inputs, size_t n_public,
                                      size_t pi_stride, const uint8_t* proofs, size_t proof_len, size_t count, const void* setup_g2,
                                      size_t g2_stride_bytes, const uint64_t* weights, uint64_t out_p1s[54], int* valid, size_t* bad_index) {
    try {
        return circuit_verify_batch_impl(ctx, key_p1s, n, t, log_ext, g, exponents, shifts, public_inputs, n_public, pi_stride, proofs,
                                         proof_len, count, setup_g2, g2_stride_bytes, weights, true, out_p1s, valid, bad_index);
    } catch (...) {
        ctx->last_error = "circuit verify batch: out of host memory or threads";
        return KZG_ERR_HIP;
    }
}

// ---- a circuit's proof in one call (DESIGN.md sections 4.25 to 4.28 and 4.30) ----------------------------------------------------
// The rounds under the transcript above, on one slot, quotient_mu held from start to end.  What lives across rounds sits in
// buffers the context keeps for this call alone (ctx->prove_buf, under quotient_mu; the pq_ws workspaces belong to the rounds, which
// may regrow them), sized for the whole proof at the start.  A lookup proof (nlk = 1, section 4.26) has two more rounds and wider
// buffers; the other kinds' layouts are the lookup's at zero width:
//   V, the values                               [ wires | PI | z | phi | m | f | T ] (f, T: the folded columns)   [ wires | PI | z ]
//   U, their unblinded coefficients             [ wires | PI | z | phi | m ]                                      [ wires | PI | z ]
//   S, the blinded copies that are committed    [ wires (n + 2 each) | m (n + 2) | z | phi (n + 3 each) ]         [ wires | z ]
//   B, the blinders they are patched with       [ b | u | c | p ]                                                 [ b | c ]
// Every column is transformed back once, here, with launch_ntt_batch, and the quotient's and the opening's bodies read U (ProveRound),
// which stays unblinded.  A lookup proof holds lookup_mu (the hash table of the multiplicities) between quotient_mu and the context's
// mutex.
namespace {
int prove_refused(kzg_ctx* ctx, const char* why) {
    ctx->last_error = std::string("circuit prove: ") + why;
    return KZG_ERR_INVALID_ARG;
}
// kind: the format of the proof, which the handle must have been created for.  wires: t columns of n values, host (stride in values)
// or device when `device`.  blinders (host, or null): section 4.24's array, a lookup proof's section 4.30's.  bad_row (or null): a
// lookup proof's
int circuit_prove_impl(kzg_ctx* ctx, const kzg_circuit* c, ProofKind kind, const uint64_t* key_p1s, const void* wires, size_t stride,
                       const uint64_t* public_inputs, size_t n_public, const uint64_t* blinders, uint8_t* out_proof, size_t* bad_row,
                       bool device) {
    const size_t nlk = kind == kProofLookup ? 1 : 0;
    const bool with_custom = kind == kProofCustom || kind == kProofNext, with_next = kind == kProofNext;
    const std::string what = nlk ? "circuit lookup prove" : "circuit prove", what_blinded = what + " (blinded)";
    // lookup_mu is taken after quotient_mu and given up after the frame has drained the stream (declared first, destroyed last)
    std::unique_lock<std::mutex> lkl(ctx->lookup_mu, std::defer_lock);
    PqCall call(ctx);
    if (!circuit_alive(ctx, c)) return circuit_foreign(ctx);
    if (nlk && !c->c_tab) return prove_refused(ctx, "the circuit was created without a lookup table");
    if (with_custom && !c->g_custom) return prove_refused(ctx, "the circuit was created without custom gates");
    if (with_custom && with_next != (c->rho != 0)) return custom_kind_refused(ctx, "circuit prove", with_next);
    if (with_next && blinders) return prove_refused(ctx, "next-row proofs are not blinded: a wire opened at two points needs a third blinder");
    const CustomRecord custom_rec = custom_record(c);
    // kzg_circuit_custom_prove (section 4.27) or, with rho more evaluations, kzg_circuit_custom_next_prove (section 4.28)
    const CustomRecord* custom = with_custom ? &custom_rec : nullptr;
    PqShape sh;
    if (!pq_shape(c->n, (size_t)1 << c->lg_ext, &sh) || stride < c->n || n_public > c->n) return KZG_ERR_INVALID_ARG;
    const size_t n = sh.n, t = c->t, e = sh.rot, lc = nlk ? c->c_tab : 0, ncoef = t + 1 + (n_public ? 1 : 0);
    for (size_t i = 0; i < n_public; i++) {
        hf::Fr v;
        if (!fr_arg_below_r(public_inputs + 4 * i, &v)) return prove_refused(ctx, "a public input is not below r");
    }
    if (blinders) {
        std::vector<hf::Fr> bl;
        if (nlk) {
            if (!lookup_blind_shape_ok(n, t, e, lc)) return lookup_blind_shape_refused(ctx, what_blinded.c_str());
        } else {
            if (!blind_shape_ok(n, t, e)) return blind_shape_refused(ctx, what_blinded.c_str());
            if (custom && !blind_custom_shape_ok(n, t, e, custom->d_max)) return blind_custom_shape_refused(ctx, what_blinded.c_str());
        }
        if (!blind_values_ok(ctx, what_blinded.c_str(), blinders, nlk ? lookup_blind_count(t, e) : blind_count(t, e), &bl))
            return KZG_ERR_INVALID_ARG;
    }
    ProofSpec sp{kind, n, t, c->lg_ext, n_public, custom ? custom->g : 0, custom ? custom->exps : nullptr,
                 with_next ? custom->exps_next : nullptr, lc};
    sp.rho = custom ? custom->rho : 0;
    sp.lay_out();
    const size_t t_len = blinders ? blind_quotient_len(n, t, e) : sh.N - n, need = blinders ? n + t + 3 : n;
    const size_t wlen = blinders ? n + kBlindWireLen : n, zlen = blinders ? n + kBlindZLen : n;
    const size_t nbw = 2 * t + nlk * kBlindMultLen, nbz = kBlindZLen + nlk * kBlindPhiLen;  // B: [ b | u ], then [ c | p ]
    if (nlk) lkl.lock();
    call.lock();
    int rc = pq_srs_status(ctx, true, need);
    if (rc == KZG_OK) rc = call.begin();
    if (rc == KZG_OK) rc = pq_srs_status(ctx, true, need);  // (the wait for a slot dropped the mutex)
    if (rc == KZG_OK) rc = ensure_ntt_batch(ctx);
    if (rc) return rc;
    std::unique_lock<std::mutex>& lk = call.lk();
    Slot& s = call.s();
    const int slot = call.slot();
    // every cross-round buffer at its size for the whole proof, before anything is enqueued (the stream is empty: PqCall)
    DevBuf &V = ctx->prove_buf[0], &U = ctx->prove_buf[1], &S = ctx->prove_buf[2], &T = ctx->prove_buf[3], &B = ctx->prove_buf[4];
    rc = V.reserve(ctx, (ncoef + 4 * nlk) * n * 32, s.stream);
    if (rc == KZG_OK) rc = U.reserve(ctx, (ncoef + 2 * nlk) * n * 32, s.stream);
    if (rc == KZG_OK) rc = T.reserve(ctx, t_len * 32, s.stream);
    if (rc == KZG_OK && blinders) rc = S.reserve(ctx, ((t + nlk) * wlen + (1 + nlk) * zlen) * 32, s.stream);
    if (rc == KZG_OK && blinders) rc = B.reserve(ctx, (nbw + nbz) * 32, s.stream);
    if (rc == KZG_OK && nlk) rc = s.gp_flags.reserve(ctx, 64);
    if (rc) return rc;
    uint32_t *d_v = V.dev(), *d_u = U.dev();
    uint32_t *d_s = blinders ? S.dev() : nullptr, *d_sm = blinders ? d_s + 8 * t * wlen : nullptr, *d_sz = blinders ? d_sm + 8 * nlk * wlen : nullptr;
    uint32_t* d_bl = blinders ? B.dev() : nullptr;
    uint32_t *d_vz = d_v + 8 * (ncoef - 1) * n, *d_uz = d_u + 8 * (ncoef - 1) * n;
    // the lookup's columns behind z (null without one)
    uint32_t *d_vphi = nlk ? d_vz + 8 * n : nullptr, *d_vm = nlk ? d_vz + 16 * n : nullptr, *d_vf = nlk ? d_vz + 24 * n : nullptr;
    uint32_t *d_vt = nlk ? d_vz + 32 * n : nullptr, *d_um = nlk ? d_uz + 16 * n : nullptr;
    const ProveRound round_base{&lk, slot, d_u, nullptr};
    const Fr30* itw = (const Fr30*)ctx->ntt_tw.p + 2 * kNttTableLen;
    const Fr30 inv_n = fr30_arg_from_mont256(hf::fr_inv(fr_pow2(sh.lg_n)));
    // `cols` columns of V -> U, one launch per pass for as many columns as the transform buffers hold
    auto to_coefficients = [&](size_t first, size_t cols) -> int {
        PqBufs w;
        int r = pq_bufs(ctx, n, cols, &w);
        if (r) return r;
        for (size_t c0 = 0; c0 < cols; c0 += w.chunk) {
            const size_t bc = cols - c0 < w.chunk ? cols - c0 : w.chunk;
            launch_ntt_batch(s.stream, d_v + 8 * (first + c0) * n, n, d_u + 8 * (first + c0) * n, n, sh.lg_n, (uint32_t)bc, itw, inv_n, w.A, w.B);
        }
        HIP_TRY(ctx, hipGetLastError());
        return KZG_OK;
    };
    const size_t np1 = sp.npoints();  // the proof's points before the evaluations: wires, ([m],) [z], ([phi],) chunks
    std::vector<uint64_t> p1s(18 * (np1 + 1)), evals(4 * sp.nevals());
    std::vector<uint8_t> proof(sp.len);
    auto put_points = [&](size_t first, size_t count) {
        for (size_t i = first; i < first + count; i++) {
            hf::P1 pt;
            std::memcpy(&pt, p1s.data() + 18 * i, sizeof pt);
            hf::p1_compress(proof.data() + 48 * i, pt);
        }
    };
    ProofWalk walk;  // every round below ends with the segment it has written absorbed and that segment's challenges drawn
    {
        hf::Sha256 st;
        sp.statement_prefix(st, key_p1s, c->shifts);
        sp.statement_finish(st, public_inputs, walk.h);
    }

    // the wires (and PI with them) to the device and to coefficients, their commitments; beta, gamma (a lookup proof: theta)
    if (device) {
        HIP_TRY(ctx, hipMemcpy2DAsync(d_v, n * 32, wires, stride * 32, n * 32, t, hipMemcpyDeviceToDevice, s.stream));
    } else {
        rc = pq_upload(ctx, lk, s.stream, d_v, (const uint64_t*)wires, n, t, stride);
        if (rc) return rc;
    }
    if (n_public) {
        HIP_TRY(ctx, hipMemsetAsync(d_v + 8 * t * n, 0, n * 32, s.stream));
        rc = copy_unlocked(ctx, lk, s.stream, d_v + 8 * t * n, public_inputs, n_public * 32, hipMemcpyHostToDevice,
                           "hipMemcpyAsync (public inputs)");
        if (rc) return rc;
    }
    if (blinders && !nlk) {  // B = [ b | c ], the front of the array
        rc = copy_unlocked(ctx, lk, s.stream, d_bl, blinders, (2 * t + kBlindZLen) * 32, hipMemcpyHostToDevice, "hipMemcpyAsync (blinders)");
        if (rc) return rc;
    }
    if (blinders && nlk) {  // B = [ b | u | c | p ] from the array's [ b | c | d | p | u ]
        const uint64_t *c_src = blinders + 4 * 2 * t, *p_src = c_src + 4 * (kBlindZLen + e - 2), *u_src = p_src + 4 * kBlindPhiLen;
        rc = copy_unlocked(ctx, lk, s.stream, d_bl, blinders, 2 * t * 32, hipMemcpyHostToDevice, "hipMemcpyAsync (blinders)");
        if (rc == KZG_OK)
            rc = copy_unlocked(ctx, lk, s.stream, d_bl + 8 * 2 * t, u_src, kBlindMultLen * 32, hipMemcpyHostToDevice, "hipMemcpyAsync (blinders)");
        if (rc == KZG_OK)
            rc = copy_unlocked(ctx, lk, s.stream, d_bl + 8 * nbw, c_src, kBlindZLen * 32, hipMemcpyHostToDevice, "hipMemcpyAsync (blinders)");
        if (rc == KZG_OK)
            rc = copy_unlocked(ctx, lk, s.stream, d_bl + 8 * (nbw + kBlindZLen), p_src, kBlindPhiLen * 32, hipMemcpyHostToDevice,
                               "hipMemcpyAsync (blinders)");
        if (rc) return rc;
    }
    rc = to_coefficients(0, ncoef - 1);
    if (rc) return rc;
    if (blinders) {
        HIP_TRY(ctx, hipMemcpy2DAsync(d_s, wlen * 32, d_u, n * 32, n * 32, t, hipMemcpyDeviceToDevice, s.stream));
        launch_blind_patch(s.stream, d_s, (uint32_t)n, t, wlen, d_bl, d_bl, kBlindWireLen, t);
        HIP_TRY(ctx, hipGetLastError());
    }
    rc = sync_unlocked(ctx, lk, s.stream, (what + " (wires)").c_str());
    if (rc == KZG_OK) rc = pq_commit_chunks(ctx, lk, slot, blinders ? d_s : d_u, wlen, t, p1s.data());
    if (rc) return rc;
    put_points(0, t);
    walk.round(sp, proof.data());

    // a lookup proof: the folded columns, the multiplicities of f in T, [m]; beta, gamma
    if (nlk) {
        const LkKernelScalars sc(walk.ch[0].l, nullptr, nullptr, lc);
        const uint32_t* tab = c->values.dev() + 8 * (2 * t + 2) * n;
        launch_lk_fold(s.stream, d_v, n, tab, tab + 8 * lc * n, (uint32_t)n, (uint32_t)lc, sc.view(), d_vf, d_vt);
        HIP_TRY(ctx, hipGetLastError());
        rc = lu_mult_enqueue(ctx, s, d_vt, n, d_vf, n, 1, n, lu_default_log_capacity(n), d_vm, nullptr);
        if (rc == KZG_OK) rc = to_coefficients(ncoef + 1, 1);
        if (rc == KZG_OK && blinders) {
            HIP_TRY(ctx, hipMemcpyAsync(d_sm, d_um, n * 32, hipMemcpyDeviceToDevice, s.stream));
            launch_blind_patch(s.stream, d_sm, (uint32_t)n, 1, wlen, d_bl + 8 * 2 * t, d_bl + 8 * 2 * t, kBlindMultLen, 1);
            HIP_TRY(ctx, hipGetLastError());
        }
        if (rc == KZG_OK) rc = sync_unlocked(ctx, lk, s.stream, "circuit lookup prove (multiplicities)");
        if (rc) return rc;
        size_t bad = (size_t)-1;
        rc = lu_mult_verdict(ctx, s, &bad);
        if (rc && bad != (size_t)-1) {
            if (bad_row) *bad_row = bad;
            ctx->last_error = "circuit lookup prove: the tuple of row " + std::to_string(bad) + " is in no row of the table";
            return KZG_ERR_REMAINDER;
        }
        if (rc == KZG_OK) rc = pq_commit_chunks(ctx, lk, slot, blinders ? d_sm : d_um, wlen, 1, p1s.data() + 18 * t);
        if (rc) return rc;
        put_points(t, 1);
        walk.round(sp, proof.data());
    }
    const hf::Fr theta = walk.ch[0] /* a lookup proof's */, beta = walk.ch[nlk], gamma = walk.ch[nlk + 1];

    // (phi, then) z on the device from the wires and the key's sigma values; phi_n = 0, z_n = 1; their commitments; alpha
    {
        uint64_t last[4];
        size_t bad = (size_t)-1;
        if (nlk) {
            rc = run_on_slot(ctx, lk, s, RunCall{kLuLookupForm, d_vf, nullptr, d_vt, d_vm, beta.l, n, 1, n}, d_vphi, last, &bad);
            if (rc) {
                if (bad_row && bad != (size_t)-1) *bad_row = bad;
                return rc;
            }
            if (std::memcmp(last, kFrZero.l, 32) != 0) {
                ctx->last_error = "circuit lookup prove: the running sum does not return to zero (phi_n != 0): the lookup does not hold";
                return KZG_ERR_REMAINDER;
            }
        }
        const RunCall perm{kGpPerm, d_v, c->values.dev() + 8 * (t + 2) * n, nullptr, nullptr, beta.l, n, t, n, c->shifts, gamma.l, sh.lg_n};
        rc = run_on_slot(ctx, lk, s, perm, d_vz, last, &bad);
        if (rc) return rc;
        if (std::memcmp(last, hf::kFrOne.l, 32) != 0) {
            ctx->last_error = "circuit prove: the grand product does not return to one (z_n != 1): the copy constraints do not hold";
            return KZG_ERR_REMAINDER;
        }
    }
    rc = to_coefficients(ncoef - 1, 1 + nlk);
    if (rc) return rc;
    if (blinders) {  // z and phi lie side by side in U and in S, c and p in B: one patch
        if (nlk) {
            HIP_TRY(ctx, hipMemcpy2DAsync(d_sz, zlen * 32, d_uz, n * 32, n * 32, 2, hipMemcpyDeviceToDevice, s.stream));
        } else {
            HIP_TRY(ctx, hipMemcpyAsync(d_sz, d_uz, n * 32, hipMemcpyDeviceToDevice, s.stream));
        }
        launch_blind_patch(s.stream, d_sz, (uint32_t)n, 1 + nlk, zlen, d_bl + 8 * nbw, d_bl + 8 * nbw, kBlindZLen, 1 + nlk);
        HIP_TRY(ctx, hipGetLastError());
    }
    rc = sync_unlocked(ctx, lk, s.stream, nlk ? "circuit lookup prove (z, phi)" : "circuit prove (z)");
    if (rc == KZG_OK) rc = pq_commit_chunks(ctx, lk, slot, blinders ? d_sz : d_uz, zlen, 1 + nlk, p1s.data() + 18 * (t + nlk));
    if (rc) return rc;
    put_points(t + nlk, 1 + nlk);
    walk.round(sp, proof.data());
    const hf::Fr alpha = walk.ch[nlk + 2];

    // the quotient (with the lookup's term) from the resident coefficients, its chunks' commitments; zeta
    const void* d_pi = n_public ? d_v + 8 * t * n : nullptr;
    const LookupRecord lookup_rec{d_vm, d_vphi, theta.l};
    const LookupRecord* lookup = nlk ? &lookup_rec : nullptr;
    uint64_t* chunk_p1s = p1s.data() + 18 * (t + 1 + 2 * nlk);
    rc = blinders ? circuit_quotient_blinded_impl(ctx, c, d_v, n, d_vz, d_pi, alpha.l, beta.l, gamma.l, blinders, T.p, chunk_p1s, true,
                                                  &round_base, custom, lookup)
                  : circuit_quotient_impl(ctx, c, d_v, n, d_vz, d_pi, alpha.l, beta.l, gamma.l, nullptr, T.p, chunk_p1s, true, &round_base,
                                          lookup, custom);
    if (rc) return rc;
    put_points(t + 1 + 2 * nlk, e - 1);
    walk.round(sp, proof.data());
    const hf::Fr zeta = walk.ch[nlk + 3];

    // the last two rounds: the evaluations, v from them, r(zeta) = 0, the opening
    ProveRound last_round = round_base;
    last_round.derive_v = [&](const uint64_t* ev, uint64_t v[4]) {
        for (size_t i = 0; i < sp.nevals(); i++) proof_fr_to_be(pq_fr(ev + 4 * i), proof.data() + sp.evals_off() + 32 * i);
        walk.round(sp, proof.data());
        std::memcpy(v, walk.ch[nlk + 4].l, 32);
        return true;
    };
    rc = circuit_open_impl(ctx, c, d_v, n, d_vz, d_pi, T.p, alpha.l, beta.l, gamma.l, zeta.l, hf::kFrOne.l /* replaced by derive_v */,
                           evals.data(), nullptr, p1s.data() + 18 * np1, true, blinders, &last_round, lookup, custom);
    if (rc) return rc;
    hf::P1 w;
    std::memcpy(&w, p1s.data() + 18 * np1, sizeof w);
    hf::p1_compress(proof.data() + sp.w_off(), w);
    std::memcpy(out_proof, proof.data(), sp.len);
    return KZG_OK;
}
// The exported prove calls: their argument checks (need_blinders: the call refuses a null array), the forwarding of a multi-device
// context to the device that holds the whole SRS (the _device forms take a single-device context), the body
static int circuit_prove_entry(kzg_ctx* ctx, const kzg_circuit* circuit, ProofKind kind, const uint64_t* key_p1s, const void* wires,
                               size_t stride, const uint64_t* public_inputs, size_t n_public, const uint64_t* blinders, bool need_blinders,
                               uint8_t* out_proof, size_t* bad_row, bool device) {
    if (bad_row) *bad_row = (size_t)-1;
    if (device) KZG_SINGLE_DEVICE_ONLY(ctx);
    if (!ctx || !circuit || !key_p1s || !wires || (!public_inputs && n_public) || (need_blinders && !blinders) || !out_proof)
        return KZG_ERR_INVALID_ARG;
    if (ctx->multi) {
        kzg_ctx* kid = whole_srs_kid(ctx, true, "the proof's commitments need");
        if (!kid) return KZG_ERR_INVALID_ARG;
        return forwarded(ctx, kid, circuit_prove_entry(kid, circuit, kind, key_p1s, wires, stride, public_inputs, n_public, blinders,
                                                       need_blinders, out_proof, bad_row, device));
    }
    return circuit_prove_impl(ctx, circuit, kind, key_p1s, wires, stride, public_inputs, n_public, blinders, out_proof, bad_row, device);
}
}  // namespace

int kzg_circuit_lookup_prove(kzg_ctx* ctx, const kzg_circuit* circuit, const uint64_t* key_p1s, const uint64_t* wires, size_t stride,
                             const uint64_t* public_inputs, size_t n_public, uint8_t* out_proof, size_t* bad_row) {
    return circuit_prove_entry(ctx, circuit, kProofLookup, key_p1s, wires, stride, public_inputs, n_public, nullptr, false, out_proof, bad_row,
                               false);
}

int kzg_circuit_lookup_prove_device(kzg_ctx* ctx, const kzg_circuit* circuit, const uint64_t* key_p1s, const void* d_wires, size_t stride,
                                    const uint64_t* public_inputs, size_t n_public, uint8_t* out_proof, size_t* bad_row) {
    return circuit_prove_entry(ctx, circuit, kProofLookup, key_p1s, d_wires, stride, public_inputs, n_public, nullptr, false, out_proof,
                               bad_row, true);
}

int kzg_circuit_lookup_prove_blinded(kzg_ctx* ctx, const kzg_circuit* circuit, const uint64_t* key_p1s, const uint64_t* wires,
                                     size_t stride, const uint64_t* public_inputs, size_t n_public, const uint64_t* blinders,
                                     uint8_t* out_proof, size_t* bad_row) {
    return circuit_prove_entry(ctx, circuit, kProofLookup, key_p1s, wires, stride, public_inputs, n_public, blinders, true, out_proof, bad_row,
                               false);
}

int kzg_circuit_lookup_prove_blinded_device(kzg_ctx* ctx, const kzg_circuit* circuit, const uint64_t* key_p1s, const void* d_wires,
                                            size_t stride, const uint64_t* public_inputs, size_t n_public, const uint64_t* blinders,
                                            uint8_t* out_proof, size_t* bad_row) {
    return circuit_prove_entry(ctx, circuit, kProofLookup, key_p1s, d_wires, stride, public_inputs, n_public, blinders, true, out_proof,
                               bad_row, true);
}

int kzg_circuit_prove(kzg_ctx* ctx, const kzg_circuit* circuit, const uint64_t* key_p1s, const uint64_t* wires, size_t stride,
                      const uint64_t* public_inputs, size_t n_public, const uint64_t* blinders, uint8_t* out_proof) {
    return circuit_prove_entry(ctx, circuit, kProofPlain, key_p1s, wires, stride, public_inputs, n_public, blinders, false, out_proof, nullptr,
                               false);
}

int kzg_circuit_prove_device(kzg_ctx* ctx, const kzg_circuit* circuit, const uint64_t* key_p1s, const void* d_wires, size_t stride,
                             const uint64_t* public_inputs, size_t n_public, const uint64_t* blinders, uint8_t* out_proof) {
    return circuit_prove_entry(ctx, circuit, kProofPlain, key_p1s, d_wires, stride, public_inputs, n_public, blinders, false, out_proof,
                               nullptr, true);
}

int kzg_circuit_custom_prove(kzg_ctx* ctx, const kzg_circuit* circuit, const uint64_t* key_p1s, const uint64_t* wires, size_t stride,
                             const uint64_t* public_inputs, size_t n_public, const uint64_t* blinders, uint8_t* out_proof) {
    return circuit_prove_entry(ctx, circuit, kProofCustom, key_p1s, wires, stride, public_inputs, n_public, blinders, false, out_proof, nullptr,
                               false);
}

int kzg_circuit_custom_prove_device(kzg_ctx* ctx, const kzg_circuit* circuit, const uint64_t* key_p1s, const void* d_wires, size_t stride,
                                    const uint64_t* public_inputs, size_t n_public, const uint64_t* blinders, uint8_t* out_proof) {
    return circuit_prove_entry(ctx, circuit, kProofCustom, key_p1s, d_wires, stride, public_inputs, n_public, blinders, false, out_proof,
                               nullptr, true);
}

int kzg_circuit_custom_next_prove(kzg_ctx* ctx, const kzg_circuit* circuit, const uint64_t* key_p1s, const uint64_t* wires, size_t stride,
                                  const uint64_t* public_inputs, size_t n_public, const uint64_t* blinders, uint8_t* out_proof) {
    return circuit_prove_entry(ctx, circuit, kProofNext, key_p1s, wires, stride, public_inputs, n_public, blinders, false, out_proof, nullptr,
                               false);
}

int kzg_circuit_custom_next_prove_device(kzg_ctx* ctx, const kzg_circuit* circuit, const uint64_t* key_p1s, const void* d_wires,
                                         size_t stride, const uint64_t* public_inputs, size_t n_public, const uint64_t* blinders,
                                         uint8_t* out_proof) {
    return circuit_prove_entry(ctx, circuit, kProofNext, key_p1s, d_wires, stride, public_inputs, n_public, blinders, false, out_proof,
                               nullptr, true);
}

int kzg_verify_points(const uint64_t commitment_p1[18], const uint64_t proof_p1[18], const uint64_t* zs, const uint64_t* ys,
                      size_t k, const void* setup_g1, size_t g1_stride_bytes, const void* setup_g2, size_t g2_stride_bytes,
                      int* valid) {
    if (!commitment_p1 || !proof_p1 || !zs || !ys || !setup_g1 || !setup_g2 || !valid) return KZG_ERR_INVALID_ARG;
    const int r = hf::verify_points(commitment_p1, proof_p1, zs, ys, k, (const uint8_t*)setup_g1, g1_stride_bytes,
                                    (const uint8_t*)setup_g2, g2_stride_bytes);
    if (r < 0) return KZG_ERR_INVALID_ARG;
    *valid = r;
    return KZG_OK;
}

// SetupArtifact k's G2 half on the host: [s^k mod r]G2 (reference src/trusted_setup.rs:40-53 for the power, :64-72 for
// the point; s = secret read big-endian, src/trusted_setup.rs:20-28)
int kzg_srs_g2_at(const uint8_t secret_be[32], uint64_t index, uint64_t out_p2[36]) {
    if (!secret_be || !out_p2) return KZG_ERR_INVALID_ARG;
    hf::Fr s;
    for (int w = 0; w < 4; w++) {
        uint64_t v = 0;
        for (int b = 0; b < 8; b++) v = (v << 8) | secret_be[24 - 8 * w + b];
        s.l[w] = v;
    }
    uint64_t br = 0;
    while (hf::fr_geq(s, hf::kFrMod)) s = hf::fr_raw_sub(s, hf::kFrMod, br);  // 2^256 < 3 r
    static const hf::Fr kR2 = {{0xc999e990f3f29c6dULL, 0x2b6cedcb87925c23ULL, 0x05d314967254398fULL, 0x0748d9d99f59ff11ULL}};
    const hf::Fr power = hf::fr_pow(hf::fr_mul(s, kR2), index);  // Montgomery form of s^index
    uint64_t e[4];
    hf::fr_from_mont(power.l, e);
    const hf::P2 q = hf::p2_normalize(hf::p2_mul(hf::p2_generator(), e));
    std::memcpy(out_p2, &q, sizeof q);
    return KZG_OK;
}

// ---- powers-of-tau ceremonies: contribute to the resident SRS, verify it ------------------------

namespace {
// secrets leave the host's memory before the call returns (a plain memset of a dying object may be dropped)
void wipe(void* p, size_t bytes) {
    volatile uint8_t* q = (volatile uint8_t*)p;
    while (bytes--) *q++ = 0;
}
struct WipeGuard {
    void* p;
    size_t bytes;
    ~WipeGuard() { wipe(p, bytes); }
};
// KZG_SRS_TRACE=1: the two calls print where their wall time went (one line on stderr each; tests/perf_srs_ceremony.py).
// A traced update waits for the device after every phase.
struct SrsTrace {
    bool on;
    std::chrono::steady_clock::time_point t;
    std::string line;
    explicit SrsTrace(const char* what) {
        const char* v = std::getenv("KZG_SRS_TRACE");
        on = v && v[0] == '1';
        if (on) {
            line = what;
            t = std::chrono::steady_clock::now();
        }
    }
    void mark(const char* phase) {
        if (!on) return;
        const auto now = std::chrono::steady_clock::now();
        char buf[96];
        std::snprintf(buf, sizeof buf, " %s_ms=%.3f", phase, std::chrono::duration<double, std::milli>(now - t).count());
        line += buf;
        t = now;
    }
    ~SrsTrace() { if (on) std::fprintf(stderr, "%s\n", line.c_str()); }
};
// 32 big-endian bytes -> the 256-bit integer as little-endian words (reference src/trusted_setup.rs:24)
void be32_to_raw8(const uint8_t be[32], uint32_t raw[8]) {
    for (int w = 0; w < 8; w++) {
        const uint8_t* b = be + 28 - 4 * w;
        raw[w] = ((uint32_t)b[0] << 24) | ((uint32_t)b[1] << 16) | ((uint32_t)b[2] << 8) | (uint32_t)b[3];
    }
}
// ... reduced mod r (2^256 < 3 r)
hf::Fr raw8_mod_r(const uint32_t raw[8]) {
    hf::Fr s;
    for (int w = 0; w < 4; w++) s.l[w] = raw[2 * w] | ((uint64_t)raw[2 * w + 1] << 32);
    uint64_t br = 0;
    while (hf::fr_geq(s, hf::kFrMod)) s = hf::fr_raw_sub(s, hf::kFrMod, br);
    return s;
}
bool g2_in_subgroup(const uint64_t raw_p2[36]) {  // [r] Q == infinity
    hf::P2 q;
    std::memcpy(&q, raw_p2, sizeof q);
    return hf::p2_mul(q, hf::kFrMod.l).is_inf();
}
}  // namespace

static int multi_replicated_only(kzg_ctx* ctx, const char* what) {
    if (multi_mode(ctx->multi) != kMultiReplicate) {
        ctx->last_error = std::string(what) + ": range-split multi-device contexts are not supported (use KZG_MULTI_REPLICATE_SRS)";
        return KZG_ERR_INVALID_ARG;
    }
    return multi_srs_len(ctx->multi) ? KZG_OK : KZG_ERR_NO_SRS;
}

int kzg_srs_update(kzg_ctx* ctx, const uint8_t tau_be[32], uint64_t first) {
    if (!ctx || !tau_be) return KZG_ERR_INVALID_ARG;
    uint32_t raw[8];
    WipeGuard wipe_raw{raw, sizeof raw};
    be32_to_raw8(tau_be, raw);
    bool zero;
    {
        hf::Fr t = raw8_mod_r(raw);
        zero = t.is_zero();
        wipe(&t, sizeof t);
    }
    if (ctx->multi) {  // a replicated SRS: every device in turn
        std::lock_guard<std::mutex> lkm(ctx->mu);
        ctx->last_error.clear();
        int rc = multi_replicated_only(ctx, "kzg_srs_update");
        if (rc) return rc;
        if (zero) {
            ctx->last_error = "kzg_srs_update: tau is zero mod r";
            return KZG_ERR_INVALID_ARG;
        }
        for (int g = 0; g < multi_num_devices(ctx->multi) && rc == KZG_OK; g++) {
            kzg_ctx* kid = multi_kid(ctx->multi, g);
            rc = forwarded(ctx, kid, kzg_srs_update(kid, tau_be, first));
        }
        return rc;
    }
    std::unique_lock<std::mutex> lk(ctx->mu);
    quiesce(ctx, lk);
    if (!ctx->n) return KZG_ERR_NO_SRS;
    if (zero) {  // a zero contribution destroys the setup
        ctx->last_error = "kzg_srs_update: tau is zero mod r";
        return KZG_ERR_INVALID_ARG;
    }
    SrsTrace tr("kzg_srs_update:");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    int rc = drain_all(ctx);
    if (rc) return rc;
    const size_t n = ctx->n;
    // the new level 0 in temporaries: the context keeps the old SRS until the kernels have succeeded
    DevBuf d_new, d_prefix, d_xyzz;
    HIP_TRY(ctx, hipMalloc(&d_new.p, n * kAffineBytes));
    HIP_TRY(ctx, hipMalloc(&d_prefix.p, n * 64));
    HIP_TRY(ctx, hipMalloc(&d_xyzz.p, n * kXyzzBytes));
    TmpStream st;
    HIP_TRY(ctx, hipStreamCreateWithFlags(&st.s, hipStreamNonBlocking));
    tr.mark("alloc");
    launch_srs_update(st.s, raw, first, (uint32_t)n, ctx->table.p, d_xyzz.p);
    if (tr.on) HIP_TRY(ctx, hipStreamSynchronize(st.s));
    tr.mark("ladder");
    launch_xyzz_to_affine(st.s, d_xyzz.p, (uint32_t)n, d_new.p, d_prefix.p);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipStreamSynchronize(st.s));
    tr.mark("normalise");
    // from here on a failure leaves the context without an SRS: everything derived from the old one goes, as in srs_prepare
    ctx->slots_ready = false;
    for (auto& s : ctx->slots) s.kind = SLOT_IDLE;
    ctx->fk20_B.reset();  // the FK20 cache holds transforms of the old SRS
    ctx->fk20_tab.reset();
    ctx->lag_table.reset();  // ... and so is the Lagrange basis (nothing in flight reads it: drained above, ctx->mu held since)
    ctx->lag_n = 0;
    ctx->srs_gen++;
    rc = hipMemcpyAsync(ctx->table.p, d_new.p, n * kAffineBytes, hipMemcpyDeviceToDevice, st.s) == hipSuccess ? KZG_OK : KZG_ERR_HIP;
    if (rc == KZG_OK) rc = build_tables(ctx, st.s, d_xyzz.p, d_prefix.p);
    else ctx->last_error = "kzg_srs_update: copying the new points into the table failed";
    if (rc) {
        ctx->table.reset();
        ctx->n = 0;
        for (auto& s : ctx->slots) free_slot_msm(s);
        (void)hipGetLastError();
        return rc;
    }
    tr.mark("tables");
    rc = setup_slots(ctx);
    tr.mark("slots");
    return rc;
}

// the steps of kzg_srs_verify that need the device; hook: the caller's weights, step 5 alone, both sums returned
// sides: B, then A (normalised blst_p1); *failed: a check before step 5 has set *reason already
static int srs_verify_device(kzg_ctx* ctx, SrsTrace& tr, const uint64_t* weights, bool hook, unsigned flags, uint64_t sides[2][18],
                             bool* failed, unsigned* reason, size_t* bad_index) {
    std::unique_lock<std::mutex> lk(ctx->mu);
    if (!ctx->n || !ctx->slots_ready) return KZG_ERR_NO_SRS;
    if (ctx->raw_partials) return KZG_ERR_INVALID_ARG;  // a device of a range-split context holds a slice, not a setup
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const int slot = reserve_slot(ctx, lk, true);
    if (slot < 0) return KZG_ERR_BUSY;
    SlotLease lease{ctx, slot};  // keeps an SRS replacement out until the call returns
    Slot& s = ctx->slots[slot];
    const size_t n = ctx->n;
    const hipStream_t st = s.stream;
    int rc = KZG_OK;
    if (!hook) {
        DevBuf d_err, d_p1;
        HIP_TRY(ctx, hipMalloc(&d_err.p, 256));
        HIP_TRY(ctx, hipMalloc(&d_p1.p, 144));
        HIP_TRY(ctx, hipMemsetAsync(d_err.p, 0xff, 8, st));
        launch_srs_check(st, ctx->table.p, (uint32_t)n, (uint32_t*)d_err.p);
        launch_affine_to_p1(st, ctx->table.p, 1, d_p1.p);
        HIP_TRY(ctx, hipGetLastError());
        uint32_t herr[2];
        uint64_t first_p1[18];
        HIP_TRY(ctx, hipMemcpyAsync(herr, d_err.p, sizeof herr, hipMemcpyDeviceToHost, st));
        HIP_TRY(ctx, hipMemcpyAsync(first_p1, d_p1.p, sizeof first_p1, hipMemcpyDeviceToHost, st));
        rc = sync_unlocked(ctx, lk, st, "srs verify");
        if (rc) return rc;
        tr.mark("subgroup_check");
        for (int e = 0; e < 2; e++)
            if (herr[e] != 0xffffffffu) {
                *reason = e ? KZG_SRS_NOT_IN_G1 : KZG_SRS_INFINITY;
                if (bad_index) *bad_index = herr[e];
                *failed = true;
                return KZG_OK;
            }
        const hf::P1 gen = hf::p1_generator();
        if ((flags & KZG_SRS_FIRST_IS_GENERATOR) && std::memcmp(first_p1, &gen, sizeof gen) != 0) {
            *reason = KZG_SRS_FIRST_NOT_GENERATOR;
            if (bad_index) *bad_index = 0;
            *failed = true;
            return KZG_OK;
        }
    }
    std::memset(sides, 0, 2 * 144);
    if (n > 1) {
        // one buffer [0, rho_0, ..., rho_(n-2), 0] of plain integers serves both sums: B is the MSM of the n scalars from
        // offset 0 (rho_(i-1) meets SRS[i]), A the one from offset 1 (rho_i meets SRS[i])
        std::vector<uint64_t> sc;
        try {
            sc.assign(4 * (n + 1), 0);
        } catch (...) {
            ctx->last_error = "srs verify: out of host memory";
            return KZG_ERR_HIP;
        }
        if (weights) {
            for (size_t i = 0; i + 1 < n; i++) hf::fr_from_mont(weights + 4 * i, &sc[4 * (i + 1)]);
        } else {  // uniform 128-bit weights from the OS, fresh on every call
            std::vector<uint64_t> rnd(2 * (n - 1));
            if (!vc_random(rnd.data(), rnd.size() * 8)) {
                ctx->last_error = std::string("srs verify: getrandom: ") + std::strerror(errno);
                return KZG_ERR_HIP;
            }
            for (size_t i = 0; i + 1 < n; i++) {
                sc[4 * (i + 1)] = rnd[2 * i];
                sc[4 * (i + 1) + 1] = rnd[2 * i + 1];
            }
        }
        DevBuf d_sc;
        HIP_TRY(ctx, hipMalloc(&d_sc.p, (n + 1) * 32));
        rc = copy_unlocked(ctx, lk, st, d_sc.p, sc.data(), (n + 1) * 32, hipMemcpyHostToDevice, "srs verify: hipMemcpyAsync (weights)");
        if (rc) return rc;
        for (int pass = 0; pass < 2 && rc == KZG_OK; pass++) {
            rc = submit_commit_locked(ctx, slot, (const uint32_t*)d_sc.p + 8 * pass, 0, n, true, true);
            if (rc) break;
            await_unlocked(lk, s);
            rc = wait_locked(ctx, slot, sides[pass]);
            s.kind = SLOT_RESERVED;  // (wait_locked left it idle under the mutex we still hold) ours until the lease ends
        }
        if (rc) {
            (void)hipStreamSynchronize(st);  // nothing reads d_sc after it is freed
            return rc;
        }
        tr.mark("msm_x2");
    }
    return KZG_OK;
}

static int srs_verify_impl(kzg_ctx* ctx, const uint64_t* weights, bool hook, const void* setup_g2, size_t g2_stride_bytes,
                           unsigned flags, uint64_t* out_a, uint64_t* out_b, int* valid, unsigned* reason, size_t* bad_index) {
    if (!ctx) return KZG_ERR_INVALID_ARG;
    const char* what = hook ? "kzg_srs_verify_lincomb" : "kzg_srs_verify";
    if (!setup_g2 || !valid || (hook ? (!out_a || !out_b) : !reason)) {
        std::lock_guard<std::mutex> lk(ctx->mu);
        ctx->last_error = std::string(what) + ": a required pointer is NULL";
        return KZG_ERR_INVALID_ARG;
    }
    *valid = 0;
    if (reason) *reason = KZG_SRS_OK;
    if (bad_index) *bad_index = (size_t)-1;
    if (ctx->multi) {  // a replicated SRS: the first device's copy
        kzg_ctx* kid = nullptr;
        {
            std::lock_guard<std::mutex> lk(ctx->mu);
            ctx->last_error.clear();
            const int rc = multi_replicated_only(ctx, what);
            if (rc) return rc;
            kid = multi_kid(ctx->multi, 0);
        }
        return forwarded(ctx, kid, srs_verify_impl(kid, weights, hook, setup_g2, g2_stride_bytes, flags, out_a, out_b, valid, reason,
                                                   bad_index));
    }
    // step 1, on the host: the two G2 points
    hf::G2Affine g2[2];
    uint64_t raw[2][36];
    for (int i = 0; i < 2; i++) {
        std::memcpy(raw[i], (const uint8_t*)setup_g2 + i * g2_stride_bytes, sizeof raw[i]);
        g2[i] = hf::g2_from_p2(raw[i]);
        if (!hf::g2_on_curve(g2[i])) {
            std::lock_guard<std::mutex> lk(ctx->mu);
            ctx->last_error = std::string(what) + ": setup_g2[" + (i ? "1" : "0") + "] is not on the twist";
            return KZG_ERR_INVALID_ARG;
        }
    }
    if (!hook) {
        const hf::G2Affine gen = hf::g2_generator();
        if (g2[0].inf || !(g2[0].x == gen.x) || !(g2[0].y == gen.y) || g2[1].inf || !g2_in_subgroup(raw[1])) {
            *reason = KZG_SRS_G2_BAD;
            return KZG_OK;
        }
    }
    size_t count = 0;
    {
        std::lock_guard<std::mutex> lk(ctx->mu);
        count = ctx->n;
        if (!count) return KZG_ERR_NO_SRS;
        if (hook && count > 1) {
            if (!weights) {
                ctx->last_error = std::string(what) + ": a required pointer is NULL";
                return KZG_ERR_INVALID_ARG;
            }
            for (size_t t = 0; t + 1 < count; t++) {
                hf::Fr v;
                std::memcpy(v.l, weights + 4 * t, 32);
                if (hf::fr_geq(v, hf::kFrMod)) {
                    ctx->last_error = std::string(what) + ": weight " + std::to_string(t) + " is not below r";
                    return KZG_ERR_INVALID_ARG;
                }
            }
        }
    }
    SrsTrace tr(hook ? "kzg_srs_verify_lincomb:" : "kzg_srs_verify:");
    uint64_t sides[2][18];
    bool failed = false;
    const int rc = srs_verify_device(ctx, tr, hook ? weights : nullptr, hook, flags, sides, &failed, reason, bad_index);
    if (rc || failed) return rc;
    if (hook) {
        std::memcpy(out_a, sides[1], 144);
        std::memcpy(out_b, sides[0], 144);
    }
    // step 5: e(A, [s]G2) == e(B, [1]G2); with one point there is nothing to compare (both sides are infinity)
    *valid = count > 1 ? vc_pair(sides[1], sides[0], g2[1], g2[0]) : 1;
    tr.mark("pairing");
    if (!*valid && reason) *reason = KZG_SRS_NOT_POWERS;
    return KZG_OK;
}

int kzg_srs_verify(kzg_ctx* ctx, const void* setup_g2, size_t g2_stride_bytes, unsigned flags, int* valid, unsigned* reason,
                   size_t* bad_index) {
    return srs_verify_impl(ctx, nullptr, false, setup_g2, g2_stride_bytes, flags, nullptr, nullptr, valid, reason, bad_index);
}

int kzg_srs_verify_lincomb(kzg_ctx* ctx, const uint64_t* weights, const void* setup_g2, size_t g2_stride_bytes,
                           uint64_t out_a_p1[18], uint64_t out_b_p1[18], int* valid) {
    return srs_verify_impl(ctx, weights, true, setup_g2, g2_stride_bytes, 0u, out_a_p1, out_b_p1, valid, nullptr, nullptr);
}

int kzg_g2_mul(const uint64_t in_p2[36], const uint8_t scalar_be[32], uint64_t out_p2[36]) {
    if (!in_p2 || !scalar_be || !out_p2) return KZG_ERR_INVALID_ARG;
    if (!hf::g2_on_curve(hf::g2_from_p2(in_p2))) return KZG_ERR_INVALID_ARG;
    uint32_t raw[8];
    WipeGuard wipe_raw{raw, sizeof raw};
    be32_to_raw8(scalar_be, raw);
    hf::Fr k = raw8_mod_r(raw);
    WipeGuard wipe_k{&k, sizeof k};
    hf::P2 q;
    std::memcpy(&q, in_p2, sizeof q);
    const hf::P2 out = hf::p2_normalize(hf::p2_mul(q, k.l));
    std::memcpy(out_p2, &out, sizeof out);
    return KZG_OK;
}

int kzg_srs_verify_update(const uint64_t before_p1[18], const uint64_t after_p1[18], const uint64_t tau_g2[36], int* valid) {
    if (!before_p1 || !after_p1 || !tau_g2 || !valid) return KZG_ERR_INVALID_ARG;
    const hf::G2Affine q = hf::g2_from_p2(tau_g2);
    if (!hf::g2_on_curve(q)) return KZG_ERR_INVALID_ARG;  // as kzg_verify_proof answers a G2 input off the twist
    *valid = 0;
    hf::P1 before, after;
    std::memcpy(&before, before_p1, sizeof before);
    std::memcpy(&after, after_p1, sizeof after);
    // a link with a point at infinity, a point off the curve or a [tau]G2 outside the subgroup of order r is no link
    if (before.is_inf() || after.is_inf() || !hf::p1_on_curve(before) || !hf::p1_on_curve(after)) return KZG_OK;
    if (q.inf || !g2_in_subgroup(tau_g2)) return KZG_OK;
    *valid = vc_pair(before_p1, after_p1, q, hf::g2_generator());  // e(before, [tau]G2) == e(after, [1]G2)
    return KZG_OK;
}

// ---- multilinear openings (multilinear_kernels.hip) ----------------------------------------------------
// Every round runs on a slot its caller holds (reserve_slot), with the context's mutex, dropping it while it copies or waits.
namespace {
bool ml_multipliers(const uint64_t* vals, size_t count, MlMultipliers* out) {  // false: one of them is not below r
    for (size_t i = 0; i < count; i++) {
        hf::Fr v;
        if (!fr_arg_below_r(vals + 4 * i, &v)) return false;
        if (out) {
            const Fr30 d = fr30_arg_from_mont256(v);
            std::memcpy(out->m[i], d.d, sizeof d.d);
        }
    }
    return true;
}
// r below r and outside {0, 1, -1}; zs: r, -r, r^2
int ml_points(const uint64_t r[4], hf::Fr zs[3]) {
    if (!fr_arg_below_r(r, &zs[0])) return KZG_ERR_INVALID_ARG;
    zs[1] = hf::fr_sub(hf::Fr{{0, 0, 0, 0}}, zs[0]);
    zs[2] = hf::fr_mul(zs[0], zs[0]);
    if (zs[0].is_zero() || zs[0] == hf::kFrOne || zs[1] == hf::kFrOne) return KZG_ERR_INVALID_ARG;
    return KZG_OK;
}
int ml_bad(kzg_ctx* ctx, const char* what, const char* why) {
    if (ctx && !ctx->multi) ctx->last_error = std::string(what) + ": " + why;
    return KZG_ERR_INVALID_ARG;
}
// the arguments the calls share, in the documented order (null where a call takes none; ptrs_ok: its other pointers)
int ml_check(kzg_ctx* ctx, const char* what, bool ptrs_ok, size_t ell, const uint64_t* us, MlMultipliers* um, const uint64_t* r,
             hf::Fr* zs, const uint64_t* gamma, hf::Fr* gf) {
    if (!ctx) return KZG_ERR_INVALID_ARG;
    if (!ptrs_ok) return ml_bad(ctx, what, "a null pointer");
    if (ell < 1 || ell > KZG_ML_MAX_VARS) return ml_bad(ctx, what, "ell must be in [1, KZG_ML_MAX_VARS]");
    if (us && !ml_multipliers(us, ell, um)) return ml_bad(ctx, what, "a coordinate of u is not below r");
    hf::Fr tmp[3];
    if (r && !fr_arg_below_r(r, &tmp[0])) return ml_bad(ctx, what, "r is not below the modulus");
    if (gamma && !fr_arg_below_r(gamma, gf)) return ml_bad(ctx, what, "gamma is not below r");
    if (r && ml_points(r, zs)) return ml_bad(ctx, what, "r is 0, 1 or -1: the points r, -r, r^2 collide");
    return KZG_OK;
}
size_t ml_level_offset(size_t n, size_t i) { return n - (n >> (i - 1)); }  // of level i >= 1 in the pyramid, in values

int ml_fold_on(kzg_ctx* ctx, std::unique_lock<std::mutex>& lk, Slot& s, const uint32_t* d_evals, size_t ell, const MlMultipliers& um,
               uint32_t* d_pyr, uint64_t* out_v) {
    const size_t n = (size_t)1 << ell;
    launch_ml_fold(s.stream, d_evals, (uint32_t)ell, um, d_pyr);
    HIP_TRY(ctx, hipGetLastError());
    int rc = KZG_OK;
    if (out_v) rc = copy_unlocked(ctx, lk, s.stream, out_v, d_pyr + 8 * (n - 2), 32, hipMemcpyDeviceToHost, "hipMemcpyAsync (v)");
    if (rc == KZG_OK) rc = sync_unlocked(ctx, lk, s.stream, "multilinear fold");
    return rc;
}
int ml_evaluations_on(kzg_ctx* ctx, std::unique_lock<std::mutex>& lk, Slot& s, const uint32_t* d_evals, const uint32_t* d_pyr,
                      size_t ell, const hf::Fr zs[3], uint64_t* out_ys) {
    const size_t n = (size_t)1 << ell;
    int rc = s.ctab.reserve(ctx, kCombineTabLen * sizeof(Fr30), s.stream);
    if (rc == KZG_OK) rc = s.cvals.reserve(ctx, kCombineMax * 32, s.stream);
    if (rc == KZG_OK) rc = s.cpart.reserve(ctx, 3 * ell * combine_tiles((uint32_t)n) * kCombinePartialWords * 4, s.stream);
    if (rc) return rc;
    Fr30* tab = (Fr30*)s.ctab.h;
    combine_fill_powers(tab, zs[0]);
    combine_fill_powers(tab + kCombineTabGamma, zs[2]);
    HIP_TRY(ctx, hipMemcpyAsync(s.ctab.d, s.ctab.h, 2 * kCombineTabGamma * sizeof(Fr30), hipMemcpyHostToDevice, s.stream));
    launch_ml_eval(s.stream, d_evals, d_pyr, (uint32_t)ell, s.ctab.dev<Fr30>(), s.cpart.dev(), s.cvals.dev());
    HIP_TRY(ctx, hipGetLastError());
    rc = sync_unlocked(ctx, lk, s.stream, "multilinear evaluations");
    if (rc == KZG_OK) std::memcpy(out_ys, s.cvals.host(), 96 * ell);
    return rc;
}
static_assert(2 * kCombineTabGamma <= kCombineTabLen && 3 * KZG_ML_MAX_VARS <= kCombineMax, "the slot's table and values hold a call");

// One MSM job per level, bit for bit kzg_commit of that level.  A second slot is borrowed when one is idle, and the levels
// alternate between the two, so that the sort of one level runs beside the accumulation of the previous one; the small levels
// take the one-launch small-job path inside enqueue_msm.
int ml_commit_folds_on(kzg_ctx* ctx, std::unique_lock<std::mutex>& lk, int slot, const uint32_t* d_pyr, size_t ell, uint64_t* out_p1s) {
    if (!ctx->n || !ctx->slots_ready) return KZG_ERR_NO_SRS;
    const size_t n = (size_t)1 << ell;
    int slots[2] = {slot, ell > 2 ? reserve_slot(ctx, lk, false) : -1};
    const int ns = slots[1] >= 0 ? 2 : 1;
    size_t pending[2] = {0, 0};  // the level in flight on each slot, 0: none
    auto collect = [&](int k) {
        Slot& q = ctx->slots[slots[k]];
        await_unlocked(lk, q);
        const int rc = wait_locked(ctx, slots[k], out_p1s + 18 * (pending[k] - 1));
        q.kind = SLOT_RESERVED;  // (wait_locked marked the slot idle under the mutex we hold; it stays this call's)
        pending[k] = 0;
        return rc;
    };
    int rc = KZG_OK;
    for (size_t i = 1; i < ell && rc == KZG_OK; i++) {
        const int k = (int)(i % (size_t)ns);
        if (pending[k]) rc = collect(k);
        if (rc) break;
        rc = submit_commit_locked(ctx, slots[k], d_pyr + 8 * ml_level_offset(n, i), 1, n >> i, false, true);
        if (rc == KZG_OK) pending[k] = i;
    }
    for (int k = 0; k < ns; k++)
        if (pending[k]) {
            const int rc2 = collect(k);  // (also after an error: nothing stays in flight)
            if (rc == KZG_OK) rc = rc2;
        }
    if (slots[1] >= 0) release_owned(ctx, slots[1]);
    return rc;
}
// F into the slot's staging buffer, then the three-point scan and the MSM of a multiproof.  The round has no claims to check:
// F's own values at the points stand in for them.
int ml_open_on(kzg_ctx* ctx, std::unique_lock<std::mutex>& lk, int slot, const uint32_t* d_evals, const uint32_t* d_pyr, size_t ell,
               const hf::Fr zs[3], const hf::Fr& gamma, uint64_t out_p1[18]) {
    if (!ctx->n || !ctx->slots_ready) return KZG_ERR_NO_SRS;
    const size_t n = (size_t)1 << ell;
    Slot& s = ctx->slots[slot];
    int rc = ensure_poly(ctx, s, n);
    if (rc) return rc;
    MlMultipliers gm;
    hf::Fr g = hf::kFrOne;
    for (size_t i = 0; i < KZG_ML_MAX_VARS; i++) {
        const Fr30 d = fr30_arg_from_mont256(g);
        std::memcpy(gm.m[i], d.d, sizeof d.d);
        g = hf::fr_mul(g, gamma);
    }
    launch_ml_combine(s.stream, d_evals, d_pyr, (uint32_t)ell, gm, s.stage.dev());
    HIP_TRY(ctx, hipGetLastError());
    uint64_t z[12], y0[12] = {};
    for (int p = 0; p < 3; p++) std::memcpy(z + 4 * p, zs[p].l, 32);
    rc = submit_points_locked(ctx, slot, s.stage.dev(), n, z, y0, 3, true);
    if (rc) return rc;
    await_unlocked(lk, s);
    s.pts_ys.assign(points_values(s, 3), points_values(s, 3) + 24);
    rc = wait_locked(ctx, slot, out_p1);
    s.kind = SLOT_RESERVED;  // (wait_locked marked the slot idle under the mutex we hold; the lease ends it)
    return rc;
}
// a call's slot: the context's mutex (lk) taken, a slot reserved, its stream there
int ml_begin(kzg_ctx* ctx, std::unique_lock<std::mutex>& lk, SlotLease& lease) {
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    lease.slot = reserve_slot(ctx, lk, true);
    if (lease.slot < 0) return KZG_ERR_BUSY;
    return ensure_slot_basics(ctx, ctx->slots[lease.slot]);
}
// the values of a host-pointer call into the slot's own buffers
int ml_upload(kzg_ctx* ctx, std::unique_lock<std::mutex>& lk, Slot& s, const uint64_t* evals, size_t n) {
    int rc = s.ml_in.reserve(ctx, n * 32, s.stream);
    if (rc == KZG_OK) rc = s.ml_pyr.reserve(ctx, n * 32, s.stream);
    if (rc == KZG_OK) rc = copy_unlocked(ctx, lk, s.stream, s.ml_in.p, evals, n * 32, hipMemcpyHostToDevice, kCopyCoeffs);
    return rc;
}
int ml_fold_host(kzg_ctx* ctx, const char* what, const uint64_t* evals, size_t ell, const uint64_t* us, uint64_t* out_pyr,
                 uint64_t* out_v) {
    MlMultipliers um;
    int rc = ml_check(ctx, what, evals && us && (out_pyr || out_v), ell, us, &um, nullptr, nullptr, nullptr, nullptr);
    if (rc) return rc;
    if (ctx->multi) {  // needs no SRS
        kzg_ctx* kid = multi_kid(ctx->multi, 0);
        return forwarded(ctx, kid, ml_fold_host(kid, what, evals, ell, us, out_pyr, out_v));
    }
    const size_t n = (size_t)1 << ell;
    std::unique_lock<std::mutex> lk(ctx->mu);
    SlotLease lease{ctx, -1};
    rc = ml_begin(ctx, lk, lease);
    if (rc) return rc;
    Slot& s = ctx->slots[lease.slot];
    rc = ml_upload(ctx, lk, s, evals, n);
    if (rc == KZG_OK && out_pyr)
        launch_ml_fold(s.stream, s.ml_in.dev(), (uint32_t)ell, um, s.ml_pyr.dev());
    if (rc == KZG_OK && out_pyr) {
        HIP_TRY(ctx, hipGetLastError());
        rc = copy_unlocked(ctx, lk, s.stream, out_pyr, s.ml_pyr.p, (n - 1) * 32, hipMemcpyDeviceToHost, "hipMemcpyAsync (pyramid)");
        if (rc == KZG_OK) rc = sync_unlocked(ctx, lk, s.stream, "multilinear fold");
    } else if (rc == KZG_OK) {
        rc = ml_fold_on(ctx, lk, s, s.ml_in.dev(), ell, um, s.ml_pyr.dev(), out_v);
    }
    return rc;
}
}  // namespace

int kzg_ml_fold(kzg_ctx* ctx, const uint64_t* evals, size_t ell, const uint64_t* us, uint64_t* out_pyramid) {
    if (ctx && !out_pyramid) return ml_bad(ctx, "kzg_ml_fold", "a null pointer");
    return ml_fold_host(ctx, "kzg_ml_fold", evals, ell, us, out_pyramid, nullptr);
}
int kzg_ml_evaluate(kzg_ctx* ctx, const uint64_t* evals, size_t ell, const uint64_t* us, uint64_t out_v[4]) {
    return ml_fold_host(ctx, "kzg_ml_evaluate", evals, ell, us, nullptr, out_v);
}

int kzg_ml_fold_device(kzg_ctx* ctx, const void* d_evals, size_t ell, const uint64_t* us, void* d_pyramid, uint64_t out_v[4]) {
    MlMultipliers um;
    int rc = ml_check(ctx, "kzg_ml_fold_device", d_evals && us && d_pyramid && out_v, ell, us, &um, nullptr, nullptr, nullptr, nullptr);
    if (rc) return rc;
    KZG_SINGLE_DEVICE_ONLY(ctx);
    std::unique_lock<std::mutex> lk(ctx->mu);
    SlotLease lease{ctx, -1};
    rc = ml_begin(ctx, lk, lease);
    if (rc) return rc;
    return ml_fold_on(ctx, lk, ctx->slots[lease.slot], (const uint32_t*)d_evals, ell, um, (uint32_t*)d_pyramid, out_v);
}

int kzg_ml_commit_folds_device(kzg_ctx* ctx, const void* d_pyramid, size_t ell, uint64_t* out_p1s) {
    int rc = ml_check(ctx, "kzg_ml_commit_folds_device", d_pyramid && (out_p1s || ell == 1), ell, nullptr, nullptr, nullptr, nullptr, nullptr,
                      nullptr);
    if (rc) return rc;
    KZG_SINGLE_DEVICE_ONLY(ctx);
    std::unique_lock<std::mutex> lk(ctx->mu);
    if (!ctx->n || !ctx->slots_ready) return KZG_ERR_NO_SRS;
    SlotLease lease{ctx, -1};
    rc = ml_begin(ctx, lk, lease);
    if (rc) return rc;
    return ml_commit_folds_on(ctx, lk, lease.slot, (const uint32_t*)d_pyramid, ell, out_p1s);
}

int kzg_ml_evaluations_device(kzg_ctx* ctx, const void* d_evals, const void* d_pyramid, size_t ell, const uint64_t r[4], uint64_t* out_ys) {
    hf::Fr zs[3];
    int rc = ml_check(ctx, "kzg_ml_evaluations_device", d_evals && d_pyramid && r && out_ys, ell, nullptr, nullptr, r, zs, nullptr, nullptr);
    if (rc) return rc;
    KZG_SINGLE_DEVICE_ONLY(ctx);
    std::unique_lock<std::mutex> lk(ctx->mu);
    SlotLease lease{ctx, -1};
    rc = ml_begin(ctx, lk, lease);
    if (rc) return rc;
    return ml_evaluations_on(ctx, lk, ctx->slots[lease.slot], (const uint32_t*)d_evals, (const uint32_t*)d_pyramid, ell, zs, out_ys);
}

int kzg_ml_open_device(kzg_ctx* ctx, const void* d_evals, const void* d_pyramid, size_t ell, const uint64_t r[4], const uint64_t gamma[4],
                       uint64_t out_p1[18]) {
    hf::Fr zs[3], gf;
    int rc = ml_check(ctx, "kzg_ml_open_device", d_evals && d_pyramid && r && gamma && out_p1, ell, nullptr, nullptr, r, zs, gamma, &gf);
    if (rc) return rc;
    KZG_SINGLE_DEVICE_ONLY(ctx);
    std::unique_lock<std::mutex> lk(ctx->mu);
    if (!ctx->n || !ctx->slots_ready) return KZG_ERR_NO_SRS;
    SlotLease lease{ctx, -1};
    rc = ml_begin(ctx, lk, lease);
    if (rc) return rc;
    return ml_open_on(ctx, lk, lease.slot, (const uint32_t*)d_evals, (const uint32_t*)d_pyramid, ell, zs, gf, out_p1);
}

int kzg_ml_open(kzg_ctx* ctx, const uint64_t* evals, size_t ell, const uint64_t* us, const uint64_t r[4], const uint64_t gamma[4],
                uint64_t out_v[4], uint64_t* out_fold_p1s, uint64_t* out_ys, uint64_t out_p1[18]) {
    MlMultipliers um;
    hf::Fr zs[3], gf;
    int rc = ml_check(ctx, "kzg_ml_open", evals && us && r && gamma && out_v && (out_fold_p1s || ell == 1) && out_ys && out_p1, ell, us, &um,
                      r, zs, gamma, &gf);
    if (rc) return rc;
    if (ctx->multi) {
        kzg_ctx* kid = whole_srs_kid(ctx, true, "kzg_ml_open needs");
        if (!kid) return KZG_ERR_INVALID_ARG;
        return forwarded(ctx, kid, kzg_ml_open(kid, evals, ell, us, r, gamma, out_v, out_fold_p1s, out_ys, out_p1));
    }
    const size_t n = (size_t)1 << ell;
    std::unique_lock<std::mutex> lk(ctx->mu);
    if (!ctx->n || !ctx->slots_ready) return KZG_ERR_NO_SRS;
    SlotLease lease{ctx, -1};
    rc = ml_begin(ctx, lk, lease);
    if (rc) return rc;
    Slot& s = ctx->slots[lease.slot];
    // the results reach the caller's memory only when every round succeeded
    uint64_t v[4], w[18];
    std::vector<uint64_t> folds(18 * (ell - 1)), ys(12 * ell);
    rc = ml_upload(ctx, lk, s, evals, n);
    if (rc == KZG_OK) rc = ml_fold_on(ctx, lk, s, s.ml_in.dev(), ell, um, s.ml_pyr.dev(), v);
    if (rc == KZG_OK) rc = ml_commit_folds_on(ctx, lk, lease.slot, s.ml_pyr.dev(), ell, folds.data());
    if (rc == KZG_OK) rc = ml_evaluations_on(ctx, lk, s, s.ml_in.dev(), s.ml_pyr.dev(), ell, zs, ys.data());
    if (rc == KZG_OK) rc = ml_open_on(ctx, lk, lease.slot, s.ml_in.dev(), s.ml_pyr.dev(), ell, zs, gf, w);
    if (rc) return rc;
    std::memcpy(out_v, v, 32);
    if (ell > 1) std::memcpy(out_fold_p1s, folds.data(), 144 * (ell - 1));
    std::memcpy(out_ys, ys.data(), 96 * ell);
    std::memcpy(out_p1, w, 144);
    return KZG_OK;
}

int kzg_ml_verify(const uint64_t commitment_p1[18], size_t ell, const uint64_t* us, const uint64_t v[4], const uint64_t* fold_p1s,
                  const uint64_t* ys, const uint64_t r[4], const uint64_t gamma[4], const uint64_t proof_p1[18], const void* setup_g1,
                  size_t g1_stride_bytes, const void* setup_g2, size_t g2_stride_bytes, int* valid) {
    if (!commitment_p1 || !us || !v || !ys || !r || !gamma || !proof_p1 || !setup_g1 || !setup_g2 || !valid) return KZG_ERR_INVALID_ARG;
    if (ell < 1 || ell > KZG_ML_MAX_VARS || (!fold_p1s && ell > 1)) return KZG_ERR_INVALID_ARG;
    hf::Fr zs[3], gf, vf;
    if (!ml_multipliers(us, ell, nullptr) || !fr_arg_below_r(r, &zs[0]) || !fr_arg_below_r(gamma, &gf) || !fr_arg_below_r(v, &vf))
        return KZG_ERR_INVALID_ARG;
    if (ml_points(r, zs)) return KZG_ERR_INVALID_ARG;
    // (*) for every level: 2 r f_(i+1)(r^2) = r (1 - u_i) (y_(i,0) + y_(i,1)) + u_i (y_(i,0) - y_(i,1)), f_ell(r^2) := v
    bool star = true;
    const hf::Fr two_r = hf::fr_add(zs[0], zs[0]);
    for (size_t i = 0; i < ell; i++) {
        hf::Fr y[3], u, next = vf;
        for (int p = 0; p < 3; p++)
            if (!fr_arg_below_r(ys + 4 * (3 * i + p), &y[p])) return KZG_ERR_INVALID_ARG;
        if (i + 1 < ell && !fr_arg_below_r(ys + 4 * (3 * (i + 1) + 2), &next)) return KZG_ERR_INVALID_ARG;
        std::memcpy(u.l, us + 4 * i, 32);
        const hf::Fr lhs = hf::fr_mul(two_r, next);
        const hf::Fr rhs = hf::fr_add(hf::fr_mul(hf::fr_mul(zs[0], hf::fr_sub(hf::kFrOne, u)), hf::fr_add(y[0], y[1])),
                                      hf::fr_mul(u, hf::fr_sub(y[0], y[1])));
        star = star && lhs == rhs;
    }
    std::vector<uint64_t> stack(18 * ell);
    std::memcpy(stack.data(), commitment_p1, 144);
    if (ell > 1) std::memcpy(stack.data() + 18, fold_p1s, 144 * (ell - 1));
    const std::vector<uint32_t> set_of(ell, 0u);
    const uint32_t set_len[1] = {3};
    uint64_t z[12];
    for (int p = 0; p < 3; p++) std::memcpy(z + 4 * p, zs[p].l, 32);
    int ok = 0;
    const int rc = kzg_verify_sets(stack.data(), ell, set_of.data(), set_len, 1, z, ys, gamma, proof_p1, setup_g1, g1_stride_bytes, setup_g2,
                                   g2_stride_bytes, &ok);
    if (rc) return rc;
    *valid = star && ok ? 1 : 0;
    return KZG_OK;
}

// ---- measurement ---------------------------------------------------------------------------------

int kzg_set_timing(kzg_ctx* ctx, int enabled) {
    KZG_SINGLE_DEVICE_ONLY(ctx);
    if (!ctx) return KZG_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(ctx->mu);
    ctx->timing = enabled != 0;
    return KZG_OK;
}
int kzg_get_times(kzg_ctx* ctx, int slot, kzg_kernel_times* out) {
    KZG_SINGLE_DEVICE_ONLY(ctx);
    if (!ctx || !out || slot < 0 || slot >= kNumSlots) return KZG_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(ctx->mu);
    *out = ctx->slots[slot].times;
    return KZG_OK;
}

}  // extern "C"
