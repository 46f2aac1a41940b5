/* kzg_mi355x.h -- C-ABI of libkzg_mi355x.so: the MI355X (gfx950) engine behind the hot path of
 * VGLoic/kzg-poly-commit-exploration, i.e. Polynomial::commit and Evaluation::generate_proof.
 *
 * The reference has no FFI seam of its own: commit / generate_proof are inherent Rust methods that
 * descend into blst one scalar multiplication at a time (reference src/polynomial.rs:200-215,
 * 260-269 -> src/curves.rs:79-96).  The boundary is therefore the BODY of those two methods; every
 * entry point below cites the reference code it replaces, and INTEGRATION.md shows the Rust
 * `extern "C"` block and the two method bodies a maintainer would write against this header.
 *
 * Layouts are blst's, so Rust passes its own memory without conversion:
 *   Fr  ("blst_fr",  reference src/scalar.rs:7-8)   : 4 x uint64 little-endian limbs, Montgomery, R = 2^256
 *   Fp  ("blst_fp")                                 : 6 x uint64 little-endian limbs, Montgomery, R = 2^384
 *   G1  ("blst_p1",  reference src/curves.rs:10-17) : {x, y, z} Jacobian, 18 x uint64; z == 0 <=> infinity
 *
 * Conventions: plain pointers and sizes only; the caller owns every buffer; the library copies what
 * it keeps and never retains a host pointer past return; every function returns 0 (KZG_OK) or a
 * negative kzg_status; nothing throws or longjmps across the boundary.  A kzg_ctx drives one GPU
 * (kzg_ctx_create; one process per GPU with the RCCL exchange in the host program, see bench.py) or several GPUs of
 * one node from one process (kzg_ctx_create_multi / _ex: SRS split by point range with an RCCL exchange of the partial
 * sums inside the library, or SRS replicated with batches split by polynomial).  Every entry point may be called
 * from several threads on the same context: the synchronous host-pointer calls (kzg_commit, kzg_open, kzg_*_batch)
 * each take one of the context's stream slots and run side by side; different contexts are independent.
 *
 * There is no CPU fallback: without a HIP device kzg_ctx_create fails with KZG_ERR_NO_DEVICE.
 */
#ifndef KZG_MI355X_H
#define KZG_MI355X_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct kzg_ctx kzg_ctx;

/* Bumped whenever a struct or a signature below changes incompatibly (2: kzg_kernel_times lost `scan_ms` in round 2;
 * 3: kzg_ctx_create_multi_ex, host-pointer batches; 4: kzg_kernel_times gained accumulate_events_ms at its end).  kzg_abi_version() returns the value the library was built
 * with: a caller compiled against another value must not read kzg_kernel_times. */
#define KZG_ABI_VERSION 4
int kzg_abi_version(void);

typedef enum kzg_status {
    KZG_OK = 0,
    /* "Setup does not allow for commitment generation of the polynomial. The polynomial degree is
     * too high."  (reference src/polynomial.rs:201-205) */
    KZG_ERR_DEGREE_TOO_HIGH = -1,
    /* "Unable to divide a constant polynomial"  (reference src/polynomial.rs:159-167) */
    KZG_ERR_CONSTANT_POLY = -2,
    /* "[divide_by_root] Fail to divide the polynomial by a root, constant terms do not add up"
     * (reference src/polynomial.rs:184-192) */
    KZG_ERR_REMAINDER = -3,
    KZG_ERR_INVALID_ARG = -4,
    KZG_ERR_NO_DEVICE = -5,  /* no usable HIP device: the library has no CPU path */
    KZG_ERR_HIP = -6,        /* a HIP runtime call failed; kzg_last_error() has the text */
    KZG_ERR_NO_SRS = -7,     /* commit/open before kzg_srs_load_g1 / kzg_srs_generate_g1 */
    KZG_ERR_BUSY = -8        /* async slot still in flight */
} kzg_status;

/* ---- context ------------------------------------------------------------------------------ */

/* Creates the engine on HIP device `device` (streams, workspaces are sized at SRS load).
 * No reference analogue: the reference is stateless and receives the SRS slice on every call
 * (src/polynomial.rs:200); the context exists to keep the SRS resident in HBM. */
int kzg_ctx_create(int device, kzg_ctx** out);
/* One context over `ndev` HIP devices of this node (the signature SURVEY.md section 8(b) sketched).  The SRS is
 * split by point range: devices[g] keeps points [g * ceil(n/ndev), ...) resident with their window tables
 * (kzg_srs_load_g1 / kzg_srs_generate_g1 on the context do the split).  kzg_commit, kzg_commit_le_bytes and kzg_open
 * then shard transparently -- one partial MSM per device driven by its own host thread; a range-sharded opening
 * evaluates the slices, runs the ndev-step carry recurrence on the host and opens every slice extended by its carry
 * (replaces the same bodies, reference src/polynomial.rs:200-215 and 260-269) -- and the 144-byte partial sums are
 * exchanged with ncclAllGather (librccl, one communicator per device, single process) and added with kzg_g1_sum:
 * RCCL has no reduction operator for curve points, so "reduce" = all-gather + K-1 complete additions.
 * A device may be listed more than once (virtual slices: how a one-GPU box rehearses the path); such a context
 * gathers on the host, since a communicator needs distinct devices (the same fallback is taken when RCCL cannot
 * form the communicator).  kzg_evaluate / kzg_quotient run on devices[0].  The host-pointer batches
 * (kzg_commit_batch / kzg_open_batch) work on every kind of context.  The asynchronous and device-pointer entry points
 * (kzg_*_submit / kzg_wait* / kzg_dev_*) name ONE device's memory and slots: they return KZG_ERR_INVALID_ARG on a
 * multi-device context, also when ndev == 1.
 *
 * kzg_ctx_create_multi_ex(..., KZG_MULTI_REPLICATE_SRS, ...): every device keeps the WHOLE SRS and work is split by
 * polynomial instead (BASELINE config 5: 64 openings of degree 2^20 on 8 GPUs): polynomial p
 * of a kzg_commit_batch / kzg_open_batch goes to devices[p mod ndev], each device pipelines its share through its
 * stream slots, nothing is exchanged.  Single kzg_commit / kzg_open calls take the devices in turn, so caller
 * threads spread over the GPUs.  flags == 0 is kzg_ctx_create_multi. */
#define KZG_MULTI_REPLICATE_SRS 1u
int kzg_ctx_create_multi(const int* devices, int ndev, kzg_ctx** out);
int kzg_ctx_create_multi_ex(const int* devices, int ndev, unsigned flags, kzg_ctx** out);
/* devices of the context (1 for kzg_ctx_create) and how many partial-sum exchanges went through RCCL so far */
int kzg_num_devices(const kzg_ctx* ctx);
uint64_t kzg_rccl_exchanges(const kzg_ctx* ctx);
void kzg_ctx_destroy(kzg_ctx* ctx);
const char* kzg_strerror(int status);
/* text of the last KZG_ERR_HIP on this context (valid until the next call on it) */
const char* kzg_last_error(const kzg_ctx* ctx);

/* ---- SRS: the G1 half of the reference's Vec<SetupArtifact> ------------------------------- */

/* Ingests n blst_p1 values starting at first_g1 with a byte stride (= size_of::<SetupArtifact>(),
 * reference src/trusted_setup.rs:31-35; the shim passes &srs[0].g1 so no field offset is
 * assumed).  Points are Jacobian with arbitrary Z as blst_p1_mult leaves them
 * (src/trusted_setup.rs:54-62); the library normalises them to affine on the device and builds
 * its window tables.  A rank of a sharded MSM loads only its slice of the SRS and commits the
 * matching coefficient slice (indices are slice-relative). */
int kzg_srs_load_g1(kzg_ctx* ctx, const void* first_g1, size_t stride_bytes, size_t n);

/* Trusted setup on the device, G1 side only: SRS[i] = [s^i mod r]G1 for i in [first, first+n),
 * s = secret read big-endian (reference src/trusted_setup.rs:20-28, 40-62).  Next-row component
 * (SURVEY.md section 8f-2); it also makes the large bench configurations set up in seconds. */
int kzg_srs_generate_g1(kzg_ctx* ctx, const uint8_t secret_be[32], uint64_t first, size_t n);

/* Wire / on-disk forms of the SRS (all of them split by range on a multi-device context):
 *  kzg_srs_load_affine      n x 96 bytes: x, y as blst_fp (Montgomery), (0, 0) = infinity -- blst_p1_affine[n].
 *                           No normalisation pass: the points go straight into the window-table builder.
 *  kzg_srs_load_compressed  n x 48 bytes, ZCash encoding: what `Serialize for G1Point` writes into the CLI's
 *                           setup.json (reference src/curves.rs:99-110) and `Deserialize` reads back with one
 *                           blst_p1_uncompress per point (src/curves.rs:112-183).  Decompressed on the device (one
 *                           lane per point: y = (x^3 + 4)^((p+1)/4), sign from the encoding); same acceptance as
 *                           blst_p1_uncompress (compressed flag, x < p, on the curve; no subgroup check).  On a
 *                           malformed point: KZG_ERR_INVALID_ARG and *bad_index = its index (bad_index may be NULL).
 *  kzg_srs_save / kzg_srs_load_file   binary cache of the resident SRS: 128-byte header ("KZGSRS1", n, compressed
 *                           first and last point as a fingerprint of the content) + n x 96-byte affine points; loading
 *                           checks the fingerprint and then takes the kzg_srs_load_affine path. */
int kzg_srs_load_affine(kzg_ctx* ctx, const void* affine_xy, size_t n);
int kzg_srs_load_compressed(kzg_ctx* ctx, const uint8_t* compressed, size_t n, size_t* bad_index);
int kzg_srs_save(kzg_ctx* ctx, const char* path);
int kzg_srs_load_file(kzg_ctx* ctx, const char* path);

/* Copies SRS entries [index, index+count) back as blst_p1 with Z = 1 (affine), e.g. to hand them
 * to the reference's serde or to check them against blst. */
int kzg_srs_read_g1(kzg_ctx* ctx, size_t index, size_t count, uint64_t* out_p1);
size_t kzg_srs_len(const kzg_ctx* ctx);

/* ---- the hot path ------------------------------------------------------------------------- */

/* Polynomial::commit (reference src/polynomial.rs:200-215): out = sum_{i<n} coeffs[i] * SRS[i].
 * coeffs = self.coefficients.as_ptr() (n x blst_fr, Montgomery).  n == 0 -> infinity.
 * n > kzg_srs_len -> KZG_ERR_DEGREE_TOO_HIGH.  out_p1 is a blst_p1 with Z = 1 (Montgomery one) or
 * all-zero for infinity, so G1Point::from(blst_p1) (src/curves.rs:13-17) wraps it directly. */
int kzg_commit(kzg_ctx* ctx, const uint64_t* coeffs_fr_mont, size_t n, uint64_t out_p1[18]);

/* Same with scalars as n x 32 canonical little-endian bytes (< r), i.e. what Scalar::to_le_bytes
 * yields (reference src/scalar.rs:83-93) and what G1Point::mult feeds blst (src/curves.rs:93).
 * Canonical input is what callers are expected to send, but it is not required: any 256-bit value is
 * accepted and counts as its residue mod r (r, v + r, 2^256 - 1 commit to the same point as their
 * reduced values; tests/test_srs_ingest_gpu.py pins this on both sort paths). */
int kzg_commit_le_bytes(kzg_ctx* ctx, const uint8_t* scalars_le, size_t n, uint64_t out_p1[18]);

/* Evaluation::generate_proof (reference src/polynomial.rs:260-269) fused on the device:
 * (P - y) (:128-145) / (x - z) (:150-195) then commit.  z = evaluation.point, y = evaluation.result
 * (4 x uint64 Montgomery each).  Error behaviour of the reference is reproduced:
 *   n == 0 and y == 0 -> infinity;  constant polynomial: c0 == y -> infinity, else
 *   KZG_ERR_CONSTANT_POLY;  P(z) != y -> KZG_ERR_REMAINDER;  quotient longer than the SRS ->
 *   KZG_ERR_DEGREE_TOO_HIGH. */
int kzg_open(kzg_ctx* ctx, const uint64_t* coeffs_fr_mont, size_t n, const uint64_t z[4],
             const uint64_t y[4], uint64_t out_p1[18]);

/* `batch` calls of Polynomial::commit / Evaluation::generate_proof against the same SRS in one call, HOST pointers:
 * polynomial p = n blst_fr values at coeffs + p * stride_coeffs * 4 (stride_coeffs >= n), result p at out_p1s + 18 * p.
 * This is the loop of the reference's callers (src/lib.rs:16-33 per polynomial; benches/evaluation_proof.rs:51-54)
 * handed over whole, so that uploads overlap kernels and, on a multi-device context, the polynomials spread over
 * the GPUs (replicated SRS: by polynomial, no communication; range-split SRS: every polynomial sharded, one
 * exchange per batch).  n <= kzg_srs_len (commit) / n - 1 <= kzg_srs_len (open): batches take truncated polynomials.
 * kzg_open_batch opens polynomial p at zs[p] with claimed value ys[p] and fills statuses[p] with KZG_OK,
 * KZG_ERR_CONSTANT_POLY or KZG_ERR_REMAINDER (out_p1s[p] is written only for KZG_OK); its return value reports
 * failures of the call as a whole.  kzg_set_max_batch bounds the polynomials per pass of the kernels (default 1). */
int kzg_commit_batch(kzg_ctx* ctx, const uint64_t* coeffs_fr_mont, size_t n, size_t batch, size_t stride_coeffs,
                     uint64_t* out_p1s /* batch x 18 */);
int kzg_open_batch(kzg_ctx* ctx, const uint64_t* coeffs_fr_mont, size_t n, size_t batch, size_t stride_coeffs,
                   const uint64_t* zs, const uint64_t* ys, uint64_t* out_p1s /* batch x 18 */, int* statuses);

/* Polynomial::sub + divide_by_root alone (reference src/polynomial.rs:128-195): writes the
 * quotient coefficients (Montgomery) to out_q (room for n-1 entries) and their count, after the
 * reference's trailing-zero truncation, to *out_qn.  Same error codes as kzg_open. */
int kzg_quotient(kzg_ctx* ctx, const uint64_t* coeffs_fr_mont, size_t n, const uint64_t z[4],
                 const uint64_t y[4], uint64_t* out_q, size_t* out_qn);

/* Polynomial::evaluate (reference src/polynomial.rs:112-123): y = P(z), the same device scan as the
 * quotient (y is its remainder).  Next-row component. */
int kzg_evaluate(kzg_ctx* ctx, const uint64_t* coeffs_fr_mont, size_t n, const uint64_t z[4],
                 uint64_t out_y[4]);

/* ---- multiproofs: one G1 element proves P at k points -------------------------------------
 * The next step of the article the reference follows (reference README.md) after single-point proofs.  With
 * Z = prod_i (X - z_i) and I the interpolant of the pairs (z_i, y_i) (degree < k), the proof is [q(s)]G1 with
 * q = (P - I) / Z, and a verifier checks  e(proof, [Z(s)]G2) == e(commitment - [I(s)]G1, G2).
 * The device computes q by partial fractions, q = sum_i w_i Q_i (Q_i the single-point quotient at z_i,
 * w_i = 1 / prod_{j != i} (z_i - z_j)): k independent scans, one MSM of n - k terms.
 * zs, ys: k x blst_fr (Montgomery), point i at zs + 4 i.
 * Arguments: 1 <= k <= KZG_MAX_OPEN_POINTS and points distinct as field elements, else (or on a NULL pointer)
 *   KZG_ERR_INVALID_ARG.  n' = n without trailing zero coefficients (the reference's truncation).
 * Errors, in kzg_open's order: any P(z_i) != y_i -> KZG_ERR_REMAINDER; otherwise n' - k > kzg_srs_len (some
 *   coefficient at index >= srs_len + k is non-zero) -> KZG_ERR_DEGREE_TOO_HIGH.  n' <= k with every claim right ->
 *   infinity (q = 0).  There is NO constant-polynomial error: a constant P gives infinity when c0 == y_i for all i
 *   and KZG_ERR_REMAINDER otherwise, where kzg_open returns KZG_ERR_CONSTANT_POLY.  For k = 1 and n' >= 2 the proof
 *   is kzg_open's bit for bit (the same kernels run).
 * Multi-device contexts: a replicated SRS forwards the call to one device; a range-split SRS returns
 *   KZG_ERR_INVALID_ARG (kzg_last_error says why).  kzg_quotient_points / kzg_evaluate_points run on devices[0]. */
#define KZG_MAX_OPEN_POINTS 64
/* host pointers, synchronous; takes one of the context's stream slots like kzg_open */
int kzg_open_points(kzg_ctx* ctx, const uint64_t* coeffs_fr_mont, size_t n, const uint64_t* zs, const uint64_t* ys,
                    size_t k, uint64_t out_p1[18]);
/* d_coeffs is a DEVICE pointer; collected by kzg_wait (single-device contexts only, like kzg_open_submit) */
int kzg_open_points_submit(kzg_ctx* ctx, int slot, const void* d_coeffs, size_t n, const uint64_t* zs,
                           const uint64_t* ys, size_t k);
/* q alone (the element-wise test hook, counterpart of kzg_quotient): out_q needs room for n - k entries; *out_qn
 * receives n' - k (0 when n' <= k).  KZG_ERR_REMAINDER as above; no SRS needed. */
int kzg_quotient_points(kzg_ctx* ctx, const uint64_t* coeffs_fr_mont, size_t n, const uint64_t* zs, const uint64_t* ys,
                        size_t k, uint64_t* out_q, size_t* out_qn);
/* the prover's first step: out_ys[4 i ..] = P(z_i), the same scans without a quotient; no SRS needed */
int kzg_evaluate_points(kzg_ctx* ctx, const uint64_t* coeffs_fr_mont, size_t n, const uint64_t* zs, size_t k,
                        uint64_t* out_ys);
/* Host only, no context (like kzg_verify_proof): reads SRS G1 entries [0, k) (blst_p1 at setup_g1 + j * g1_stride_bytes)
 * and the G2 powers [s^j]G2, j in [0, k] (blst_p2 at setup_g2 + j * g2_stride_bytes): the Rust shim passes &srs[0].g1
 * and &srs[0].g2 of its Vec<SetupArtifact> with stride size_of::<SetupArtifact>().  *valid = 1 accepted, 0 rejected.
 * KZG_ERR_INVALID_ARG for k out of range, equal points, a G1 input off the curve or a G2 input off the twist (no
 * subgroup checks, as kzg_verify_proof).  Cost: k G1 and k + 1 G2 scalar multiplications and one two-pair pairing. */
int kzg_verify_points(const uint64_t commitment_p1[18], const uint64_t proof_p1[18], const uint64_t* zs, const uint64_t* ys,
                      size_t k, const void* setup_g1, size_t g1_stride_bytes, const void* setup_g2, size_t g2_stride_bytes,
                      int* valid);

/* ---- combined openings: t polynomials at one point, one G1 element -------------------------
 * The transpose of a multiproof, and what a proof-system prover sends in its last round (PLONK and its relatives): the
 * t values y_i = P_i(z) and ONE proof, [q(s)]G1 with q = (F - F(z)) / (X - z) for F = sum_{i<t} gamma^i P_i.  A verifier
 * forms C = sum gamma^i C_i and y = sum gamma^i y_i (kzg_combine_claims) and checks the single opening (C, z, y, proof)
 * with any of the verifiers of this header; the two points z and z w of a PLONK proof are two such records in one
 * kzg_verify_proof_batch / kzg_verify_openings_batch call.
 * SOUNDNESS: gamma has to be a challenge fixed AFTER the commitments and the values y_i (and z after the commitments), as
 * the protocol's transcript defines it.  Nothing is hashed here: these calls take z and gamma as given.
 * Layout: polynomial i is n blst_fr values at coeffs + 4 i stride (stride >= n when t > 1), as kzg_open_batch takes them;
 * shorter polynomials are padded with zeros.  z, gamma: blst_fr (Montgomery), refused when not below r.
 * Prover: out_ys[4 i ..] = P_i(z).  There is no claim, hence no remainder error.  n' = F's length without trailing zero
 *   coefficients (the reference's truncation): n' <= 1 gives infinity (also when F vanishes by cancellation; there is no
 *   constant-polynomial error, as kzg_open_points); n' - 1 > kzg_srs_len gives KZG_ERR_DEGREE_TOO_HIGH.  t = 0,
 *   t > KZG_MAX_COMBINE, a NULL pointer, or stride < n with t > 1 give KZG_ERR_INVALID_ARG.  For t = 1 and n' >= 2 the
 *   proof is kzg_open's bit for bit, whatever gamma is.
 * Cost: one streaming pass over the t n coefficients (k_combine_eval: F and the t values, every coefficient read once),
 *   then the scan and the MSM of ONE opening -- where kzg_open_batch runs t scans and t MSMs.  Measured at n = 2^20 on
 *   resident inputs (profiles/r14_open_combined.jsonl, medians of 3): 3.03 / 2.89 / 3.09 / 4.21 ms per call at t = 1 / 4 / 16 /
 *   64, against 3.01 / 10.4 / 40.8 / 160.8 ms for t x kzg_open_submit through the slots (0.99 / 3.6 / 13.2 / 38.1 x);
 *   k_combine_eval with its finish kernel takes 0.06 / 0.13 / 0.42 / 1.49 ms of it, 1.08 - 1.47 TB/s of algorithmic bytes.
 * The host-pointer call uploads and combines at most kzg_max_batch(ctx) polynomials per pass (F is carried between the
 *   passes; the result does not depend on the grouping) and is bound by the upload; the resident call takes all t in one
 *   launch.
 * Multi-device contexts: a replicated SRS forwards the call to one device; a range-split SRS returns
 *   KZG_ERR_INVALID_ARG (kzg_last_error says why).  kzg_combine_polys / kzg_evaluate_batch_at run on devices[0]. */
#define KZG_MAX_COMBINE 256
/* host pointers, synchronous; takes one of the context's stream slots like kzg_open */
int kzg_open_combined(kzg_ctx* ctx, const uint64_t* coeffs_fr_mont, size_t n, size_t t, size_t stride_coeffs,
                      const uint64_t z[4], const uint64_t gamma[4], uint64_t* out_ys /* t x 4 */, uint64_t out_p1[18]);
/* d_coeffs is a DEVICE pointer; collected by kzg_wait_combined, which returns the t values of the slot's job (out_ys: t x 4)
 * and the proof (single-device contexts only, like kzg_open_points_submit) */
int kzg_open_combined_submit(kzg_ctx* ctx, int slot, const void* d_coeffs, size_t n, size_t t, size_t stride_coeffs,
                             const uint64_t z[4], const uint64_t gamma[4]);
int kzg_wait_combined(kzg_ctx* ctx, int slot, uint64_t* out_ys, uint64_t out_p1[18]);
/* with kzg_set_timing: the duration of the last job's combination pass on the slot (k_combine_eval and its finish kernel),
 * next to what kzg_get_times reports for the scan and the MSM */
int kzg_get_combine_ms(kzg_ctx* ctx, int slot, float* out_ms);
/* the element-wise test hooks, no SRS needed: F's n coefficients (canonical blst_fr) / out_ys[4 i ..] = P_i(z) */
int kzg_combine_polys(kzg_ctx* ctx, const uint64_t* coeffs_fr_mont, size_t n, size_t t, size_t stride_coeffs,
                      const uint64_t gamma[4], uint64_t* out_f);
int kzg_evaluate_batch_at(kzg_ctx* ctx, const uint64_t* coeffs_fr_mont, size_t n, size_t t, size_t stride_coeffs,
                          const uint64_t z[4], uint64_t* out_ys);
/* Host only, no context (like kzg_verify_proof).  kzg_combine_claims: C = sum gamma^i C_i (Horner in gamma: t - 1 scalar
 * multiplications, spread over up to min(hardware threads, t) threads; normalised) and y = sum gamma^i y_i.  No curve or
 * subgroup check of its own: the pair goes to a verifier, which applies its checks.  1 <= t <= KZG_MAX_COMBINE, gamma and
 * the y_i below r, else KZG_ERR_INVALID_ARG.  kzg_verify_combined: kzg_combine_claims, then kzg_verify_proof. */
int kzg_combine_claims(const uint64_t* commitments_p1, const uint64_t* ys, size_t t, const uint64_t gamma[4],
                       uint64_t out_commitment_p1[18], uint64_t out_y[4]);
int kzg_verify_combined(const uint64_t* commitments_p1, const uint64_t* ys, size_t t, const uint64_t z[4],
                        const uint64_t gamma[4], const uint64_t proof_p1[18], const uint64_t s_g2[36], int* valid);

/* ---- openings at several point sets: polynomial i on set S_g(i), one G1 element ---------------
 * The general last round of a proof-system prover: PLONK opens most polynomials at z and the permutation polynomial at
 * z w; systems with custom gates open groups at {z}, {z, z w}, {z, z w, z w^-1}.  One kzg_open_combined per point set costs
 * one MSM and one G1 element per set; these calls prove "polynomial i takes these values on S_(set_of[i])" for all i with
 * ONE MSM and ONE element (Boneh-Drake-Fisch-Gabizon 2020, the first scheme): the proof is [h(s)]G1 with
 *        h = sum_g (F_g - R_g) / Z_(S_g),      F_g = sum_{i in set g} gamma^i P_i,  R_g its interpolant on S_g.
 * kzg_open_points (t = 1, m = 1) and kzg_open_combined (one set of one point) are special cases, with the same proof bytes.
 * SOUNDNESS: gamma has to be a challenge fixed AFTER the commitments and the values (and the points after the
 * commitments), as the protocol's transcript defines it.  Nothing is hashed here: these calls take the points and gamma
 * as given.
 * Layout: polynomials as for kzg_open_combined (equal n, polynomial i at coeffs + 4 i stride, shorter ones padded with
 *   zeros).  set_of: t indices below m.  set_len: the m set sizes.  zs: sum(set_len) x blst_fr (Montgomery), set after set.
 *   The weight of polynomial i is gamma^i (i its index in the call, gamma^0 = 1 also for gamma = 0).  out_ys: polynomial
 *   after polynomial, the set_len[set_of[i]] values of polynomial i in its set's point order (sum_i set_len[set_of[i]] x 4).
 * Errors, in this order: a NULL pointer other than the coefficients; t outside [1, KZG_MAX_COMBINE]; m outside [1, KZG_MAX_SETS]; an empty set (or one
 *   of more than KZG_MAX_SET_POINTS points); set_of[i] >= m; a set no polynomial uses; a point not below r; two equal points
 *   within one set (the same point in several sets, at any position, is the normal case); more than KZG_MAX_SET_POINTS
 *   distinct points over all sets; gamma not below r; NULL coefficients with n > 0; too many coefficients; stride < n with t > 1 -- all
 *   KZG_ERR_INVALID_ARG, and kzg_last_error says which.  There is no claim, hence no remainder error.  n' = h's length
 *   without trailing zero coefficients: n' = 0 gives infinity (n <= min |S_g|, or h vanishing by cancellation);
 *   n' > kzg_srs_len gives KZG_ERR_DEGREE_TOO_HIGH.  deg h = n - 1 - min |S_g| when nothing cancels.
 * Cost: with T the distinct points over all sets, one streaming pass per point p of T over the polynomials opened at p
 *   (k_sets_combine: G_p = sum gamma^i w_(g(i),p) P_i and the values P_i(p), every such coefficient read once), |T| suffix
 *   scans summed into h (k_sets_chunks / k_sets_apply), ONE MSM.  Measured at n = 2^20 on resident inputs in PLONK's
 *   shape (nine polynomials at z, one at z w; profiles/r15_open_sets.jsonl): 3.28 ms per call (3.17-3.40 over nine alternated repetitions) against 5.33 ms
 *   (5.29-5.62) for kzg_open_combined_submit of the nine plus kzg_open_submit of the tenth in two slots, both in flight
 *   -- 1.63 x, a difference of 2.06 ms against a min-max spread of 0.33 ms of the two-call route; of the call, 0.32 ms
 *   are the two passes, 0.21 ms the two scans and 2.65 ms the MSM.  Sixteen polynomials over {z}, {z, z w},
 *   {z, z w, z / w}: 3.66 ms (passes 0.74 ms, scans 0.28 ms, MSM 2.47 ms).
 * The host-pointer call uploads at most kzg_max_batch(ctx) polynomials at a time (every G_p is carried between the groups;
 *   the result does not depend on the grouping); the resident call runs each pass over all its polynomials in one launch.
 *   Workspace per slot, grown on demand: |T| n values for the G_p.
 * Multi-device contexts: a replicated SRS forwards the call to one device; a range-split SRS returns
 *   KZG_ERR_INVALID_ARG (kzg_last_error says why).  kzg_quotient_sets runs on devices[0]. */
#define KZG_MAX_SETS 8          /* point sets per call */
#define KZG_MAX_SET_POINTS 16   /* distinct points over all sets, |T| */
/* host pointers, synchronous; takes one of the context's stream slots like kzg_open */
int kzg_open_sets(kzg_ctx* ctx, const uint64_t* coeffs_fr_mont, size_t n, size_t t, size_t stride_coeffs,
                  const uint32_t* set_of /* t */, const uint32_t* set_len /* m */, size_t m,
                  const uint64_t* zs /* sum(set_len) x 4, set after set */, const uint64_t gamma[4], uint64_t* out_ys,
                  uint64_t out_p1[18]);
/* d_coeffs is a DEVICE pointer; collected by kzg_wait_sets, which returns the values of the slot's job and the proof
 * (single-device contexts only).  kzg_wait and kzg_wait_combined refuse such a slot and leave the job in it; kzg_wait_sets
 * refuses every other kind.  With kzg_set_timing, kzg_get_combine_ms reports the passes and kzg_get_times the scans
 * (quotient_ms) and the MSM. */
int kzg_open_sets_submit(kzg_ctx* ctx, int slot, const void* d_coeffs, size_t n, size_t t, size_t stride_coeffs,
                         const uint32_t* set_of, const uint32_t* set_len, size_t m, const uint64_t* zs,
                         const uint64_t gamma[4]);
int kzg_wait_sets(kzg_ctx* ctx, int slot, uint64_t* out_ys, uint64_t out_p1[18]);
/* test hook, no SRS: h's coefficients (room for n - 1), *out_hn = length without trailing zeros, and the values */
int kzg_quotient_sets(kzg_ctx* ctx, const uint64_t* coeffs_fr_mont, size_t n, size_t t, size_t stride_coeffs,
                      const uint32_t* set_of, const uint32_t* set_len, size_t m, const uint64_t* zs, const uint64_t gamma[4],
                      uint64_t* out_ys, uint64_t* out_h, size_t* out_hn);
/* Host only, no context.  Per set g: v_(g,p) = sum_{i in g} gamma^i y_(i,p), R_g their interpolant, A_g = sum_{i in g}
 * gamma^i C_i - [R_g(s)]G1 (SRS G1 entries [0, max |S_g|), as kzg_verify_points takes them), B_g = [Z_(T \ S_g)(s)]G2 and
 * B_T = [Z_T(s)]G2 (the G2 powers [s^j]G2, j <= |T|).  *valid = 1 iff prod_g e(A_g, B_g) == e(proof, B_T): one Miller loop
 * over m + 1 <= 9 pairs, one final exponentiation, t G1 and at most (m + 1)(|T| + 1) G2 scalar multiplications.  ys in
 * out_ys' layout.  KZG_ERR_INVALID_ARG for the argument errors above, a value not below r, a G1 input off the curve or a G2
 * input off the twist (no subgroup checks, as kzg_verify_points). */
int kzg_verify_sets(const uint64_t* commitments_p1, size_t t, const uint32_t* set_of, const uint32_t* set_len, size_t m,
                    const uint64_t* zs, const uint64_t* ys, const uint64_t gamma[4], const uint64_t proof_p1[18],
                    const void* setup_g1, size_t g1_stride_bytes, const void* setup_g2, size_t g2_stride_bytes, int* valid);

/* ---- multilinear polynomials: opening the multilinear extension of 2^ell values (Gemini / HyperKZG) ----------------
 * Sum-check based provers hold a polynomial as its n = 2^ell values on the boolean hypercube and have to prove
 * f~(u) = v for a point u in Fr^ell.  Variable x_i is bit i of the index (little-endian):
 *        f~(u) = sum_j f[j] prod_i (bit_i(j) ? u_i : 1 - u_i).
 * The commitment is kzg_commit(f): the values read as the coefficients of a univariate f_0 of length n.
 * Folds, i = 0 .. ell - 1:   f_(i+1)[j] = f_i[2j] + u_i (f_i[2j+1] - f_i[2j]),  j < n / 2^(i+1);   f_ell is the one value v.
 * With f_i(X) = E_i(X^2) + X O_i(X^2), f_(i+1) = (1 - u_i) E_i + u_i O_i, hence for any r != 0
 *        2 r f_(i+1)(r^2) = r (1 - u_i) (f_i(r) + f_i(-r)) + u_i (f_i(r) - f_i(-r)).                                   (*)
 * The proof: the ell - 1 commitments C_1 .. C_(ell-1) of f_1 .. f_(ell-1); the 3 ell values y_(i,0) = f_i(r), y_(i,1) =
 * f_i(-r), y_(i,2) = f_i(r^2), i < ell, in that order; one G1 element W, bit for bit the proof of kzg_open_sets over
 * [f_0 | f_1 | .. | f_(ell-1)], each padded with zeros to n, with the one set {r, -r, r^2} and the weights gamma^i
 * (= kzg_open_points of F = sum_i gamma^i f_i at the three points).  The verifier checks (*) for every i with
 * f_ell(r^2) := v and runs kzg_verify_sets on [C, C_1 .. C_(ell-1)], the one set, the values, gamma and W.
 * SOUNDNESS: r has to be drawn after C_1 .. C_(ell-1), gamma after the values.  Nothing is hashed here: the calls take
 * u, r and gamma as given.
 * The pyramid: f_1 .. f_ell packed in one buffer of n - 1 values, level i at offset n - (n >> (i - 1)) (f_ell = v last).
 * All values and scalars are blst_fr images, fully reduced.
 * Errors, in this order: a NULL context or pointer; ell outside [1, KZG_ML_MAX_VARS]; a u_i, r or gamma not below r; r in
 *   {0, 1, r - 1} (the three points collide) -- all KZG_ERR_INVALID_ARG, nothing is written.  Then, where an SRS is needed,
 *   KZG_ERR_NO_SRS; a fold longer than kzg_srs_len with a non-zero value beyond it gives KZG_ERR_DEGREE_TOO_HIGH as kzg_commit
 *   does; W follows kzg_open_points: its quotient has n - 3 coefficients, a non-zero one at index >= kzg_srs_len gives
 *   KZG_ERR_DEGREE_TOO_HIGH.  ell = 1 has no fold commitments and W = infinity; all-zero values give infinity everywhere.
 * Cost: the folds are two launches at any ell (k_ml_fold: eleven levels per launch inside 2048-value tiles), the values one
 *   pass over f_0 and the pyramid plus a finish launch, F one pass, W one three-point scan and one MSM.  The ell - 1 fold
 *   commitments are one MSM job each, two of the context's slots alternating so that consecutive levels overlap; the small
 *   levels take the one-launch small-job path.  Measured at ell = 20 on resident values (profiles/r31_multilinear.jsonl): the
 *   four rounds 12.5 ms -- fold 0.16, fold commitments 8.6, values 0.21, W 3.0 -- against 64.8 ms (55.8-77.6) for the folds on
 *   16 host threads, one kzg_commit per level and kzg_open_sets of the padded stack from host memory.
 * Multi-device contexts: kzg_ml_fold / kzg_ml_evaluate run on devices[0]; kzg_ml_open is forwarded to one device of a
 *   replicated SRS and refused (KZG_ERR_INVALID_ARG) on a range-split one; the device forms take single-device contexts. */
#define KZG_ML_MAX_VARS 22
/* no SRS needed: the whole pyramid ((n - 1) x 4), or only v */
int kzg_ml_fold(kzg_ctx* ctx, const uint64_t* evals_fr_mont, size_t ell, const uint64_t* us /* ell x 4 */,
                uint64_t* out_pyramid /* (n - 1) x 4 */);
int kzg_ml_evaluate(kzg_ctx* ctx, const uint64_t* evals_fr_mont, size_t ell, const uint64_t* us, uint64_t out_v[4]);
/* One call per prover round over DEVICE buffers the caller holds (kzg_dev_alloc): d_evals n values, d_pyramid n - 1 values,
 * neither overlapping the other; nothing is recomputed or copied between the rounds.  Synchronous. */
int kzg_ml_fold_device(kzg_ctx* ctx, const void* d_evals, size_t ell, const uint64_t* us, void* d_pyramid, uint64_t out_v[4]);
int kzg_ml_commit_folds_device(kzg_ctx* ctx, const void* d_pyramid, size_t ell, uint64_t* out_p1s /* (ell - 1) x 18 */);
int kzg_ml_evaluations_device(kzg_ctx* ctx, const void* d_evals, const void* d_pyramid, size_t ell, const uint64_t r[4],
                              uint64_t* out_ys /* 3 ell x 4 */);
int kzg_ml_open_device(kzg_ctx* ctx, const void* d_evals, const void* d_pyramid, size_t ell, const uint64_t r[4],
                       const uint64_t gamma[4], uint64_t out_p1[18]);
/* host pointers, synchronous, the whole proof: uploads once and runs the four rounds */
int kzg_ml_open(kzg_ctx* ctx, const uint64_t* evals_fr_mont, size_t ell, const uint64_t* us, const uint64_t r[4],
                const uint64_t gamma[4], uint64_t out_v[4], uint64_t* out_fold_p1s /* (ell - 1) x 18 */,
                uint64_t* out_ys /* 3 ell x 4 */, uint64_t out_p1[18]);
/* Host only, no context: (*) for every i in host arithmetic, then kzg_verify_sets (three G1 rows, the G2 powers up to s^3).
 * *valid = 1 iff both hold; a failing (*) gives *valid = 0, not an error.  v and the values have to be below r, the points
 * decode and lie on the curve as kzg_verify_sets asks, else KZG_ERR_INVALID_ARG. */
int kzg_ml_verify(const uint64_t commitment_p1[18], size_t ell, const uint64_t* us, const uint64_t v[4],
                  const uint64_t* fold_p1s /* (ell - 1) x 18 */, const uint64_t* ys /* 3 ell x 4 */, const uint64_t r[4],
                  const uint64_t gamma[4], const uint64_t proof_p1[18], const void* setup_g1, size_t g1_stride_bytes,
                  const void* setup_g2, size_t g2_stride_bytes, int* valid);

/* ---- polynomials in evaluation form: NTT over power-of-two domains ------------------------
 * Most KZG data (blob-style commitments, proof systems) holds a polynomial as its values over a subgroup of roots of
 * unity.  These entry points take those values directly; until now a caller had to interpolate on the host first.
 * Domain of size n = 2^k, 0 <= k <= 22 (the largest SRS): {w_n^i}, w_n = 7^((r - 1) / n) mod r, 7 the multiplicative
 * generator blst, c-kzg and EIP-4844 use.  NATURAL order on both sides: evals[i] = P(w_n^i) for P = sum_j c[j] X^j.
 * Nothing is bit-reversed at the boundary: a caller holding bit-reversed values (c-kzg's blob order) permutes them on
 * the host first.  Every scalar is a blst_fr image (Montgomery), outputs fully reduced.
 * Errors: n not a power of two or above 2^22 -> KZG_ERR_INVALID_ARG.  The commit / open calls treat the interpolated
 * coefficients exactly as kzg_commit / kzg_open do (n above kzg_srs_len with a non-zero coefficient beyond it ->
 * KZG_ERR_DEGREE_TOO_HIGH, a wrong y -> KZG_ERR_REMAINDER); z may lie inside or outside the domain.
 * Multi-device contexts: kzg_ntt runs on devices[0]; the commit / open calls forward to one device of a replicated SRS
 * and return KZG_ERR_INVALID_ARG on a range-split one. */
#define KZG_NTT_MAX_LOG 22
/* host only: w_n for n = 2^log_n, log_n <= 32 (out: blst_fr) */
int kzg_domain_root(unsigned log_n, uint64_t out_mont[4]);
/* out = NTT(in) (inverse = 0: coefficients -> evaluations) or its inverse (inverse != 0, includes the 1/n);
 * host arrays of n blst_fr, in == out allowed; synchronous; no SRS needed.  Replaces the host interpolation a caller
 * with evaluations had to run before kzg_commit. */
int kzg_ntt(kzg_ctx* ctx, const uint64_t* in, size_t n, int inverse, uint64_t* out);
/* the same on kzg_dev_alloc buffers of the context's GPU (single-device contexts); d_in == d_out allowed; returns when
 * the result is in d_out */
int kzg_ntt_device(kzg_ctx* ctx, const void* d_in, void* d_out, size_t n, int inverse);
/* kzg_ntt of `batch` columns in one call: column b is the n blst_fr at in + 4 b in_stride u64 and its transform goes to
 * out + 4 b out_stride u64, bit for bit what kzg_ntt gives for that column; the strides are in values, and the values
 * between two columns (strides above n) are neither read nor written.  Every pass of the transform is one launch for the
 * columns in flight (k_nttb_pass), where kzg_ntt per column makes one launch per column and pass.
 * in == out with equal strides is allowed; any other overlap of the two sides, a stride below n, kzg_ntt's argument errors
 * and extents beyond the address space -> KZG_ERR_INVALID_ARG.  batch == 0 does nothing.  Synchronous; no SRS needed.  The
 * two intermediate buffers (and the staging buffer of the host form) come from the quotient calls' workspaces: a quarter of
 * their budget each (KZG_PQ_WS_KB) and at most 64 columns, so a larger batch runs in several rounds with the same result,
 * and the call takes its turn with the quotient calls of the context.  Multi-device contexts run it on devices[0]. */
int kzg_ntt_batch(kzg_ctx* ctx, const uint64_t* in, size_t n, size_t batch, size_t in_stride, int inverse, uint64_t* out,
                  size_t out_stride);
/* host only, a test hook: the rounds kzg_ntt_batch / kzg_ntt_batch_device take for `batch` columns of n values on this context,
 * ceil(batch / min(64, budget / (4 n 32))), 0 for an empty batch; the budget is read from KZG_PQ_WS_KB when the context is made.
 * It exists so that a test can see that a small budget really splits a batch; a caller has no need of it. */
int kzg_ntt_batch_rounds(kzg_ctx* ctx, size_t n, size_t batch, size_t* rounds);
/* the same on kzg_dev_alloc buffers of the context's GPU (single-device contexts): nothing crosses PCIe; returns when the
 * result is in d_out */
int kzg_ntt_batch_device(kzg_ctx* ctx, const void* d_in, size_t n, size_t batch, size_t in_stride, void* d_out, size_t out_stride,
                         int inverse);
/* kzg_commit of the interpolated coefficients, bit for bit: one upload, the inverse NTT into the slot's staging
 * buffer, the same MSM */
int kzg_commit_evaluations(kzg_ctx* ctx, const uint64_t* evals_fr_mont, size_t n, uint64_t out_p1[18]);
/* d_evals is a DEVICE pointer; collected by kzg_wait (single-device contexts only, like kzg_commit_submit) */
int kzg_commit_evaluations_submit(kzg_ctx* ctx, int slot, const void* d_evals, size_t n);
/* kzg_open of the interpolated coefficients at z, claimed value y (P(w_n^i) = evals[i] for z in the domain) */
int kzg_open_evaluations(kzg_ctx* ctx, const uint64_t* evals_fr_mont, size_t n, const uint64_t z[4], const uint64_t y[4],
                         uint64_t out_p1[18]);

/* ---- a Lagrange-basis SRS: commitments and openings straight from the values -------------------
 * For the domain of n = 2^log_n points (w_n as kzg_domain_root, natural order) the context can hold the Lagrange form of its
 * setup, L_i = [l_i(s)] G1 = (1/n) sum_j w^(-ij) SRS[j], with window-table levels of its own (a second W x n x 128 bytes of
 * device memory).  A commitment to values is then sum_i evals[i] L_i and an opening is the MSM of the quotient's VALUES
 * q_i = (f_i - y) / (w^i - z) over the same points (the entry with w^i = z from the others): no inverse NTT runs.  ONE basis
 * (one n) is held per context.  Every SRS load, generation, kzg_srs_update and failed load drops it; it is never rebuilt
 * behind the caller's back except by the host-pointer calls below, which build the basis of their n on first use.
 * The basis is an inverse G1 DFT of the setup and uses the endomorphism, as kzg_g1_dft does: the SRS must lie in G1
 * (kzg_srs_verify checks this).
 * Errors common to the calls on values: n not a power of two or above 2^KZG_NTT_MAX_LOG -> KZG_ERR_INVALID_ARG; no SRS ->
 * KZG_ERR_NO_SRS; n > kzg_srs_len -> KZG_ERR_DEGREE_TOO_HIGH.  This differs from kzg_commit_evaluations, which accepts
 * values of a low-degree polynomial over a domain longer than the SRS: here every one of the n basis points is a
 * combination of SRS[0 .. n), so the SRS must reach n points whatever the degree.
 * Results equal kzg_commit_evaluations / kzg_open_evaluations of the same input bit for bit (the same group element,
 * normalised the same way), with the same statuses in the same order: all n values equal (n = 1 included) -> infinity when
 * y is that value, else KZG_ERR_CONSTANT_POLY; P(z) != y -> KZG_ERR_REMAINDER, for z inside and outside the domain.
 * Multi-device contexts: a replicated SRS forwards to the device the evaluation calls forward to; a range-split one returns
 * KZG_ERR_INVALID_ARG (kzg_last_error says why); the _submit calls take single-device contexts only. */
/* builds the basis of 2^log_n points, replacing a held one of another size (waits for the jobs in flight first).
 * log_n > KZG_NTT_MAX_LOG -> KZG_ERR_INVALID_ARG; no SRS -> KZG_ERR_NO_SRS; 2^log_n > kzg_srs_len -> KZG_ERR_DEGREE_TOO_HIGH */
int kzg_lagrange_prepare(kzg_ctx* ctx, unsigned log_n);
/* points of the held basis, 0 when none is held */
size_t kzg_lagrange_len(const kzg_ctx* ctx);
/* L_index .. L_(index + count - 1) as blst_p1 with Z = 1, all zero for infinity, like kzg_srs_read_g1; KZG_ERR_NO_SRS when no
 * basis is held */
int kzg_lagrange_read_g1(kzg_ctx* ctx, size_t index, size_t count, uint64_t* out_p1);
/* upload -> MSM over the basis; builds the basis of n points on first use */
int kzg_commit_lagrange(kzg_ctx* ctx, const uint64_t* evals_fr_mont, size_t n, uint64_t out_p1[18]);
/* d_evals is a DEVICE pointer; collected by kzg_wait.  Never builds: KZG_ERR_NO_SRS unless a basis of exactly n points is held */
int kzg_commit_lagrange_submit(kzg_ctx* ctx, int slot, const void* d_evals, size_t n);
/* polynomial b by its n values at evals + 4 b stride (stride >= n, in blst_fr), result b at out_p1s + 18 b: through the batched
 * MSM in sub-batches of at most kzg_max_batch polynomials; builds the basis on first use */
int kzg_commit_lagrange_batch(kzg_ctx* ctx, const uint64_t* evals_fr_mont, size_t n, size_t batch, size_t stride, uint64_t* out_p1s);
/* the proof that P(z) = y for P given by its values; z inside or outside the domain; builds the basis on first use */
int kzg_open_lagrange(kzg_ctx* ctx, const uint64_t* evals_fr_mont, size_t n, const uint64_t z[4], const uint64_t y[4],
                      uint64_t out_p1[18]);
/* d_evals is a DEVICE pointer that stays untouched until kzg_wait collected the job; never builds, like the commit form */
int kzg_open_lagrange_submit(kzg_ctx* ctx, int slot, const void* d_evals, size_t n, const uint64_t z[4], const uint64_t y[4]);
/* test hook: the n values of the quotient the opening commits to (all zero for a constant polynomial whose claim holds); needs
 * no SRS; the statuses of kzg_open_lagrange */
int kzg_quotient_lagrange(kzg_ctx* ctx, const uint64_t* evals_fr_mont, size_t n, const uint64_t z[4], const uint64_t y[4],
                          uint64_t* out_q_evals);

/* adopts a basis GIVEN as n x 48 bytes (compressed points; order KZG_ORDER_NATURAL: point i is L_i, KZG_ORDER_BIT_REVERSED:
 * point i is L_brp(i), the order the first ceremony files carried g1_lagrange in) for the resident SRS, replacing a held one.
 * Points are decoded on the device with the subgroup check always on: a point that does not decode or lies outside G1 ->
 * KZG_ERR_INVALID_ARG with *bad_index its index in the input ((size_t)-1 otherwise; bad_index may be NULL), nothing adopted.
 * check != 0 compares the points with the resident SRS: n weights rho of 128 bits from getrandom(2), the MSM of rho over the
 * given points against the MSM of the inverse NTT of rho over the monomial table; *consistent (required then) = 1 or 0.  On 0
 * the basis is NOT adopted, a held one stays, and the call still returns KZG_OK.  A wrong basis passes with probability about
 * 2^-128.  check == 0 adopts unchecked (*consistent stays 0).  No SRS -> KZG_ERR_NO_SRS; n > kzg_srs_len -> KZG_ERR_DEGREE_TOO_HIGH */
int kzg_lagrange_load_compressed(kzg_ctx* ctx, const uint8_t* in48, size_t n, unsigned order, int check, size_t* bad_index,
                                 int* consistent);
/* a setup that exists only in Lagrange form: decodes as above, SRS[j] = sum_i w^(ij) L_i by a forward G1 DFT, then the normal
 * ingest (kzg_srs_len = n afterwards) and the decoded points stay as the Lagrange basis.  A malformed input leaves the
 * context as it was.  Single-device contexts only (KZG_ERR_INVALID_ARG otherwise) */
int kzg_srs_load_lagrange_compressed(kzg_ctx* ctx, const uint8_t* in48, size_t n, unsigned order, size_t* bad_index);

/* ---- grand products: the running product of a permutation argument --------------------------------
 * t numerator columns a_j and t denominator columns b_j of n values each.  With A_i = prod_j a_j[i] and B_i = prod_j b_j[i]:
 *     z_0 = 1,   z_(i+1) = z_i A_i / B_i   (i < n),   last = z_n.
 * Computed as z_i = (prod_{k<i} A_k) (prod_{k>=i} B_k) / (prod_k B_k): two product scans and ONE field inversion per call.
 * Column j starts at base + 4 j stride u64 (stride >= n, in blst_fr, the kzg_commit_lagrange_batch convention); every scalar is
 * a blst_fr image, outputs fully reduced; z_0 is exactly the image of one.  1 <= t <= KZG_GP_MAX_COLUMNS, 1 <= n <=
 * 2^KZG_NTT_MAX_LOG, else KZG_ERR_INVALID_ARG.  A zero numerator is legal (z is zero after it, last = 0).  A zero denominator
 * B_i -> KZG_ERR_INVALID_ARG with *bad_index the least such i ((size_t)-1 otherwise; bad_index may be NULL), kzg_last_error names
 * it, and the outputs are unspecified.
 * The permutation form (n a power of two, else KZG_ERR_INVALID_ARG; w = kzg_domain_root(log2 n), natural order) takes wire
 * columns f_j, permutation columns sigma_j -- sigma_j[i] is the label k_j' w^i' of the cell that (j, i) maps to --, the t coset
 * shifts k_j and the challenges beta, gamma:  a_j[i] = f_j[i] + beta k_j w^i + gamma,  b_j[i] = f_j[i] + beta sigma_j[i] + gamma.
 * The a_j, b_j are formed in registers, never stored.
 * The host-pointer forms are synchronous, need no SRS and run on devices[0] of a multi-device context. */
#define KZG_GP_MAX_COLUMNS 16
/* out_z: n blst_fr (z_0 .. z_(n-1)); out_last: z_n */
int kzg_grand_product(kzg_ctx* ctx, const uint64_t* nums, const uint64_t* dens, size_t n, size_t t, size_t stride, uint64_t* out_z,
                      uint64_t out_last[4], size_t* bad_index);
/* the same on kzg_dev_alloc buffers of the context's GPU (single-device contexts); d_out_z may overlap neither input
 * (KZG_ERR_INVALID_ARG); returns when z is in d_out_z, so that kzg_commit_lagrange_submit(slot, d_out_z, n) can follow */
int kzg_grand_product_device(kzg_ctx* ctx, const void* d_nums, const void* d_dens, size_t n, size_t t, size_t stride, void* d_out_z,
                             uint64_t out_last[4], size_t* bad_index);
/* the permutation form; shifts: t blst_fr */
int kzg_permutation_product(kzg_ctx* ctx, const uint64_t* wires, const uint64_t* sigmas, size_t n, size_t t, size_t stride,
                            const uint64_t* shifts, const uint64_t beta[4], const uint64_t gamma[4], uint64_t* out_z,
                            uint64_t out_last[4], size_t* bad_index);
/* ... on device buffers, as kzg_grand_product_device; shifts, beta, gamma stay host pointers */
int kzg_permutation_product_device(kzg_ctx* ctx, const void* d_wires, const void* d_sigmas, size_t n, size_t t, size_t stride,
                                   const uint64_t* shifts, const uint64_t beta[4], const uint64_t gamma[4], void* d_out_z,
                                   uint64_t out_last[4], size_t* bad_index);
/* upload -> z -> its commitment over the Lagrange basis of the n-domain, on one slot: out_p1 equals kzg_commit_lagrange of the
 * same z bit for bit.  out_z may be NULL.  Builds the basis on first use; statuses and multi-device rules of
 * kzg_commit_lagrange (no SRS -> KZG_ERR_NO_SRS, n > kzg_srs_len -> KZG_ERR_DEGREE_TOO_HIGH, a range-split context ->
 * KZG_ERR_INVALID_ARG) */
int kzg_permutation_commit(kzg_ctx* ctx, const uint64_t* wires, const uint64_t* sigmas, size_t n, size_t t, size_t stride,
                           const uint64_t* shifts, const uint64_t beta[4], const uint64_t gamma[4], uint64_t* out_z,
                           uint64_t out_last[4], uint64_t out_p1[18], size_t* bad_index);

/* ---- log-derivative (LogUp) lookup arguments: running sums, a batch inverse, multiplicities -----------
 * t numerator columns a_j and t denominator columns b_j of n values each:
 *     phi_0 = 0,   phi_(i+1) = phi_i + sum_j a_j[i] / b_j[i]   (i < n),   last = phi_n.
 * The row's fractions are added as one pair (N_i, D_i) and 1 / D_i = (prod_{k<i} D_k) (prod_{k>i} D_k) / (prod_k D_k): two product
 * scans, one additive scan and ONE field inversion per call.  Conventions of kzg_grand_product: column j starts at base + 4 j stride
 * u64 (stride >= n); every scalar is a blst_fr image, canonical in, fully reduced out; phi_0 is exactly the image of zero.
 * 1 <= t <= KZG_LOGUP_MAX_COLUMNS, 1 <= n <= 2^KZG_NTT_MAX_LOG, else KZG_ERR_INVALID_ARG.  A zero numerator is legal.  A zero
 * denominator b_j[i] -> KZG_ERR_INVALID_ARG with *bad_index the least such row i ((size_t)-1 otherwise; bad_index may be NULL),
 * kzg_last_error names the row, and the outputs are unspecified.
 * The host-pointer forms are synchronous, need no SRS and run on devices[0] of a multi-device context.  The _device forms take
 * kzg_dev_alloc buffers of a single-device context, refuse an output that overlaps an input (KZG_ERR_INVALID_ARG) and return when
 * the output is in place, so that kzg_commit_lagrange_submit(slot, d_out, n) can follow. */
#define KZG_LOGUP_MAX_COLUMNS 16
/* general form; nums == NULL: every numerator is one.  out_phi: n blst_fr (phi_0 .. phi_(n-1)), out_last: phi_n */
int kzg_logderivative_sum(kzg_ctx* ctx, const uint64_t* nums, const uint64_t* dens, size_t n, size_t t, size_t stride, uint64_t* out_phi,
                          uint64_t out_last[4], size_t* bad_index);
int kzg_logderivative_sum_device(kzg_ctx* ctx, const void* d_nums, const void* d_dens, size_t n, size_t t, size_t stride, void* d_out_phi,
                                 uint64_t out_last[4], size_t* bad_index);
/* lookup form: k lookup columns f_j (1 <= k <= KZG_LOGUP_MAX_COLUMNS - 1), one table column T and its multiplicities m, n rows
 * each, a challenge beta:
 *     phi_(i+1) = phi_i + sum_j 1 / (beta + f_j[i])  -  m_i / (beta + T_i);
 * the k + 1 denominators are formed in registers, never stored; beta + f_j[i] = 0 or beta + T_i = 0 is a zero denominator.  The
 * result equals kzg_logderivative_sum on the explicit columns limb for limb.  A lookup that holds gives last = 0; a non-zero last
 * is returned, not reported as an error */
int kzg_lookup_sum(kzg_ctx* ctx, const uint64_t* lookups, size_t n, size_t k, size_t stride, const uint64_t* table, const uint64_t* mult,
                   const uint64_t beta[4], uint64_t* out_phi, uint64_t out_last[4], size_t* bad_index);
/* ... on device buffers; beta stays a host pointer */
int kzg_lookup_sum_device(kzg_ctx* ctx, const void* d_lookups, size_t n, size_t k, size_t stride, const void* d_table, const void* d_mult,
                          const uint64_t beta[4], void* d_out_phi, uint64_t out_last[4], size_t* bad_index);
/* upload -> phi -> its commitment over the Lagrange basis of the n-domain on one slot (n a power of two, else
 * KZG_ERR_INVALID_ARG): the twin of kzg_permutation_commit, same statuses and multi-device rules; out_p1 equals
 * kzg_commit_lagrange of the same phi bit for bit; out_phi may be NULL */
int kzg_lookup_commit(kzg_ctx* ctx, const uint64_t* lookups, size_t n, size_t k, size_t stride, const uint64_t* table, const uint64_t* mult,
                      const uint64_t beta[4], uint64_t* out_phi, uint64_t out_last[4], uint64_t out_p1[18], size_t* bad_index);
/* out_i = 1 / v_i with the call's one inversion; a zero v_i -> KZG_ERR_INVALID_ARG with *bad_index the least such i */
int kzg_batch_inverse(kzg_ctx* ctx, const uint64_t* vals, size_t n, uint64_t* out, size_t* bad_index);
int kzg_batch_inverse_device(kzg_ctx* ctx, const void* d_vals, size_t n, void* d_out, size_t* bad_index);
/* Multiplicities through a hash table on the device.  table: n_table values (1 <= n_table <= 2^KZG_NTT_MAX_LOG), lookups: k
 * columns (1 <= k <= KZG_LOGUP_MAX_COLUMNS - 1) of n values (1 <= n <= 2^KZG_NTT_MAX_LOG).  out_mult[r] (the blst_fr image of a
 * count, n_table of them) = how many of the k n looked-up values equal table[r], counted at the LEAST row holding that value: later
 * duplicates of a table value get 0.  out_rows (k n uint32, column-major, or NULL): that row for every looked-up value.  Values
 * are compared as the 32 bytes given (canonical images).  A value that is in no row -> KZG_ERR_INVALID_ARG, *bad_index = the
 * least row i of the lookup columns holding one, and the outputs are unspecified */
int kzg_lookup_multiplicities(kzg_ctx* ctx, const uint64_t* table, size_t n_table, const uint64_t* lookups, size_t n, size_t k, size_t stride,
                              uint64_t* out_mult, uint32_t* out_rows, size_t* bad_index);
/* ... on device buffers (d_out_rows may be NULL); the outputs overlap no input and not each other */
int kzg_lookup_multiplicities_device(kzg_ctx* ctx, const void* d_table, size_t n_table, const void* d_lookups, size_t n, size_t k,
                                     size_t stride, void* d_out_mult, void* d_out_rows, size_t* bad_index);
/* test hook: the same with the hash table's capacity given as 2^log_capacity >= n_table, log_capacity <= KZG_NTT_MAX_LOG + 1 (the
 * public call uses the least power of two >= 2 n_table) */
int kzg_lookup_multiplicities_cap(kzg_ctx* ctx, const uint64_t* table, size_t n_table, const uint64_t* lookups, size_t n, size_t k,
                                  size_t stride, uint64_t* out_mult, uint32_t* out_rows, size_t* bad_index, unsigned log_capacity);

/* ---- the quotient of a permutation argument on a coset ------------------------------------------------
 * n = 2^k, H = <w_n> (w_n = kzg_domain_root(k)), e = 2^x with x <= KZG_PQ_MAX_LOG_EXT, N = e n <= 2^KZG_NTT_MAX_LOG.  The coset
 * points are x_i = g w_N^i with g = 7, in natural order (the coset kzg_recover_cells_and_proofs works on).  With t wire columns
 * f_j, t permutation columns sigma_j, shifts k_j, the accumulator z of kzg_permutation_product (z(w^i) = z_i, z_0 = 1) and the
 * challenges alpha, beta, gamma:
 *     Num(X) = G(X) + alpha   [ z(X) prod_j (f_j(X) + beta k_j X + gamma)  -  z(w X) prod_j (f_j(X) + beta sigma_j(X) + gamma) ]
 *                   + alpha^2 (z(X) - 1) L_0(X),              L_0(X) = (X^n - 1) / (n (X - 1)),
 *     T(X)   = Num(X) / (X^n - 1).
 * G is the caller's own term (gates, public inputs, lookups) as N values on the coset, or NULL for 0.  On the coset z(w x_i) is
 * z's value at index (i + e) mod N, and Z_H(x_i) = g^n w_e^(i mod e) - 1 takes e values, never zero.  With every column of degree
 * < n, deg Num <= (t + 1)(n - 1): e >= t + 1, so t <= KZG_PQ_MAX_COLUMNS.  Num is divisible by X^n - 1 exactly when the
 * interpolant of Num(x_i) / Z_H(x_i) has zero coefficients at [N - n, N); a non-zero one there -> KZG_ERR_REMAINDER (the
 * constraints do not hold on H), kzg_last_error says so, and the outputs are unspecified.
 * Every scalar is a blst_fr image, outputs fully reduced; columns follow the stride convention of kzg_grand_product (column j at
 * base + 4 j stride u64).  The host-pointer forms are synchronous; those that need no SRS run on devices[0] of a multi-device
 * context.  The _device forms take kzg_dev_alloc buffers of a single-device context, return when the output is written, and
 * their output may overlap no input (KZG_ERR_INVALID_ARG).  n = 1 is legal everywhere. */
#define KZG_PQ_MAX_COLUMNS 7
#define KZG_PQ_MAX_LOG_EXT 3
#define KZG_EXTEND_VALUES 0 /* len = 2^k values over the len-domain */
#define KZG_EXTEND_COEFFS 1 /* any 1 <= len <= N coefficients (e.g. a blinded polynomial of degree >= n) */
/* `batch` columns of len entries (column b at in + 4 b stride, stride >= len) -> their N = 2^log_out values on the coset, column
 * b at out + 4 b N.  len <= N (len = N: a plain coset transform).  Needs no SRS.  Anything else -> KZG_ERR_INVALID_ARG */
int kzg_coset_extend(kzg_ctx* ctx, const uint64_t* in, size_t len, size_t batch, size_t stride, unsigned form, unsigned log_out,
                     uint64_t* out);
int kzg_coset_extend_device(kzg_ctx* ctx, const void* d_in, size_t len, size_t batch, size_t stride, unsigned form,
                            unsigned log_out, void* d_out);
/* out[i] = Num(x_i) / Z_H(x_i), i < N = rot n, from the columns' N values on the coset (wires_ext / sigmas_ext: t columns, stride
 * >= N; z_ext, gate_coset, out: N values; gate_coset may be NULL).  n and rot = N / n are given apart from the columns' degrees,
 * so that columns extended from KZG_EXTEND_COEFFS (blinded, rot = 8) go through the same call.  1 <= t, t + 1 <= rot <= 8. */
int kzg_permutation_constraints_coset(kzg_ctx* ctx, const uint64_t* wires_ext, const uint64_t* sigmas_ext, const uint64_t* z_ext,
                                      size_t n, size_t rot, size_t t, size_t stride, const uint64_t* shifts, const uint64_t alpha[4],
                                      const uint64_t beta[4], const uint64_t gamma[4], const uint64_t* gate_coset, uint64_t* out);
int kzg_permutation_constraints_coset_device(kzg_ctx* ctx, const void* d_wires_ext, const void* d_sigmas_ext, const void* d_z_ext,
                                             size_t n, size_t rot, size_t t, size_t stride, const uint64_t* shifts,
                                             const uint64_t alpha[4], const uint64_t beta[4], const uint64_t gamma[4],
                                             const void* d_gate_coset, void* d_out);
/* N values of any Num on the coset -> the N - n coefficients of Num / (X^n - 1) (N / n = 2^x, x <= 3; n = N: none).
 * already_divided != 0: the values are Num(x_i) / Z_H(x_i) already (what the call above returns).  KZG_ERR_REMAINDER as above */
int kzg_vanishing_quotient(kzg_ctx* ctx, const uint64_t* num_coset, size_t N, size_t n, int already_divided, uint64_t* out_coeffs);
int kzg_vanishing_quotient_device(kzg_ctx* ctx, const void* d_num_coset, size_t N, size_t n, int already_divided,
                                  void* d_out_coeffs);
/* The whole step on one slot: wires, sigmas (t columns of n values, stride >= n) and z (n values) are extended to N = 2^log_ext n
 * points, the constraints are evaluated and divided, and T comes back as out_coeffs (NULL, or N - n coefficients) and as the
 * commitments of its chunks of n coefficients, out_p1s (NULL, or (2^log_ext - 1) x 18 u64): chunk c = coefficients
 * [c n, (c + 1) n), committed over the monomial SRS, bit for bit kzg_commit of that chunk.  gate_coset: NULL or N values.
 * Nothing but the inputs and the outputs asked for crosses PCIe.
 * KZG_ERR_INVALID_ARG: n not a power of two, N > 2^KZG_NTT_MAX_LOG, t = 0, t + 1 > 2^log_ext, log_ext > KZG_PQ_MAX_LOG_EXT,
 * stride < n, a NULL required pointer.  With out_p1s: no SRS -> KZG_ERR_NO_SRS, n > kzg_srs_len -> KZG_ERR_DEGREE_TOO_HIGH, and
 * kzg_commit_lagrange's multi-device rules (a replicated context forwards, a range-split one -> KZG_ERR_INVALID_ARG). */
int kzg_permutation_quotient(kzg_ctx* ctx, const uint64_t* wires, const uint64_t* sigmas, const uint64_t* z, size_t n, size_t t,
                             size_t stride, const uint64_t* shifts, const uint64_t alpha[4], const uint64_t beta[4],
                             const uint64_t gamma[4], const uint64_t* gate_coset, unsigned log_ext, uint64_t* out_coeffs,
                             uint64_t* out_p1s);

/* ---- a circuit's key resident on the device: the quotient with the arithmetic gate built in -----------
 * Domain, coset and notation are those above.  A circuit has t wire columns, KZG_CIRCUIT_MIN_COLUMNS <= t <= KZG_PQ_MAX_COLUMNS,
 * t linear selectors q_0 .. q_(t-1), a multiplication selector q_M, a constant selector q_C and t permutation columns sigma_j with
 * shifts k_j.  With the wires f_j, public inputs PI (n values over H, or NULL; added as given: textbook PLONK passes -x_i) and an
 * optional term G' of the caller's (N values on the coset, or NULL: lookups, custom gates):
 *     Gate(X) = sum_j q_j(X) f_j(X) + q_M(X) f_0(X) f_1(X) + q_C(X) + PI(X) + G'(X)
 *     Num(X)  = Gate(X) + alpha [ z(X) prod_j (f_j + beta k_j X + gamma) - z(w X) prod_j (f_j + beta sigma_j + gamma) ]
 *                       + alpha^2 (z(X) - 1) L_0(X),          T(X) = Num(X) / (X^n - 1).
 * The gate's degree is 3 (n - 1) <= (t + 1)(n - 1), so e >= t + 1 as above, and the divisibility test is the same.
 *
 * kzg_circuit_create uploads the 2 t + 2 columns ONCE (q_lin, sigmas: t columns of n values, column j at base + 4 j stride u64;
 * q_mul, q_const: n values) and keeps, in device buffers of the circuit's own, three forms of each -- the n values, the n
 * coefficients and the N = 2^log_ext n values on the coset -- with the N coset values of L_0 and the e inverses of Z_H.  EVERY
 * resident column, in every form, is stored as blst_fr images (the coset form is bit for bit what kzg_coset_extend returns).
 * Device memory: (2 t + 3) N x 32 bytes on the coset plus 2 (2 t + 2) n x 32 bytes of values and coefficients; at n = 2^20,
 * e = 4, t = 3 that is 9 x 128 MiB + 2 x 8 x 32 MiB = 1.625 GiB.  The columns are ordered q_lin[0..t), q_mul, q_const,
 * sigma[0..t): within each form they are contiguous at stride n (N for the coset form), so ONE kzg_open_combined_submit or
 * kzg_open_sets_submit over the coefficient form covers all the selectors, all the sigmas, or all 2 t + 2 columns.
 * out_key_p1s: NULL, or (2 t + 2) x 18 u64 that receive the commitments of the columns in that order, each bit for bit
 * kzg_commit_evaluations of the column (batched MSMs, kzg_max_batch columns per job).
 * KZG_ERR_INVALID_ARG: t < 2, t > KZG_PQ_MAX_COLUMNS, t + 1 > 2^log_ext, log_ext > KZG_PQ_MAX_LOG_EXT, n not a power of two,
 * N > 2^KZG_NTT_MAX_LOG, stride < n, a NULL required pointer.  With out_key_p1s: no SRS -> KZG_ERR_NO_SRS, n > kzg_srs_len ->
 * KZG_ERR_DEGREE_TOO_HIGH, and kzg_commit_lagrange's multi-device rules (a range-split context -> KZG_ERR_INVALID_ARG).  On a
 * multi-device context the circuit lives on devices[0] and the handle remembers it.  A failed call leaves nothing allocated and
 * *out NULL.  kzg_ctx_destroy frees the circuits still alive on the context; kzg_circuit_destroy waits for a running quotient.
 *
 * kzg_circuit_quotient extends only what changes per proof -- the t wires (t columns of n values, stride >= n), z and PI -- and
 * returns T as kzg_permutation_quotient does: out_coeffs (NULL, or N - n coefficients) and out_p1s (NULL, or (e - 1) x 18 u64, the
 * commitments of the chunks of n coefficients, bit for bit kzg_commit of each chunk).  KZG_ERR_REMAINDER when the gate or the
 * permutation does not hold on H.  A circuit made on another context -> KZG_ERR_INVALID_ARG.  With out_p1s: KZG_ERR_NO_SRS,
 * KZG_ERR_DEGREE_TOO_HIGH and the multi-device rules as above.  The _device form takes kzg_dev_alloc buffers of a single-device
 * context (d_wires, d_z, d_public_inputs: values over H; d_gate_coset: N values), returns when T's N - n coefficients are in
 * d_out_coeffs, and its output may overlap no input.
 *
 * kzg_circuit_column_device hands out a resident column, read-only: which = KZG_CIRCUIT_COL_QLIN + j, KZG_CIRCUIT_COL_QM,
 * KZG_CIRCUIT_COL_QC, KZG_CIRCUIT_COL_SIGMA + j (j < t) or KZG_CIRCUIT_COL_L0 (coset form only); *len receives n or N.  The
 * pointer is valid until the circuit is destroyed and belongs to the device the circuit lives on. */
typedef struct kzg_circuit kzg_circuit;
#define KZG_CIRCUIT_MIN_COLUMNS 2
#define KZG_CIRCUIT_COL_QLIN 0
#define KZG_CIRCUIT_COL_QM 16
#define KZG_CIRCUIT_COL_QC 17
#define KZG_CIRCUIT_COL_SIGMA 32
#define KZG_CIRCUIT_COL_L0 48
#define KZG_CIRCUIT_VALUES 0
#define KZG_CIRCUIT_COEFFS 1
#define KZG_CIRCUIT_COSET 2
int kzg_circuit_create(kzg_ctx* ctx, const uint64_t* q_lin, const uint64_t* q_mul, const uint64_t* q_const, const uint64_t* sigmas,
                       size_t n, size_t t, size_t stride, const uint64_t* shifts, unsigned log_ext, uint64_t* out_key_p1s,
                       kzg_circuit** out);
int kzg_circuit_destroy(kzg_ctx* ctx, kzg_circuit* circuit);
int kzg_circuit_quotient(kzg_ctx* ctx, const kzg_circuit* circuit, const uint64_t* wires, size_t stride, const uint64_t* z,
                         const uint64_t* public_inputs, const uint64_t alpha[4], const uint64_t beta[4], const uint64_t gamma[4],
                         const uint64_t* gate_coset, uint64_t* out_coeffs, uint64_t* out_p1s);
int kzg_circuit_quotient_device(kzg_ctx* ctx, const kzg_circuit* circuit, const void* d_wires, size_t stride, const void* d_z,
                                const void* d_public_inputs, const uint64_t alpha[4], const uint64_t beta[4],
                                const uint64_t gamma[4], const void* d_gate_coset, void* d_out_coeffs);
int kzg_circuit_column_device(kzg_ctx* ctx, const kzg_circuit* circuit, unsigned which, unsigned form, const void** d_ptr,
                              size_t* len);

/* ---- a circuit's proof, last round: linearise, open once, verify ---------------------------------------
 * Notation as above; e = 2^log_ext, w = kzg_domain_root(log2 n), T_c = coefficients [c n, (c + 1) n) of the N - n that
 * kzg_circuit_quotient returns, PI(X) the interpolant of the public inputs.  With the evaluations
 *     abar_j = f_j(zeta) (j < t),    sbar_j = sigma_j(zeta) (j < t - 1),    zw = z(zeta w)
 * and A = prod_(j<t) (abar_j + beta k_j zeta + gamma), B = zw prod_(j<t-1) (abar_j + beta sbar_j + gamma), Z = zeta^n - 1,
 * l = L_0(zeta) (the polynomial's value: Z / (n (zeta - 1)), 1 at zeta = 1; zeta in H is legal), the linearisation polynomial is
 *     r(X) = sum_j abar_j q_j(X) + abar_0 abar_1 q_M(X) + q_C(X) + (alpha A + alpha^2 l) z(X) - alpha beta B sigma_(t-1)(X)
 *            - Z sum_(c<e-1) zeta^(c n) T_c(X) + [ PI(zeta) - alpha B (abar_(t-1) + gamma) - alpha^2 l ],
 * n coefficients, and r(zeta) = 0 exactly when T is the quotient of these wires and this z.  The proof is the ONE G1 element of
 * kzg_open_sets over the 2 t + 1 polynomials [ r | f_0 .. f_(t-1) | sigma_0 .. sigma_(t-2) | z ], set_of = [0, .., 0, 1], sets
 * {zeta}, {zeta w}, gamma := v -- bit for bit what kzg_open_sets returns on that stack (for n = 1, w = 1: one point).
 * SOUNDNESS: beta and gamma are fixed after the wires' commitments, alpha after [z], zeta after the [T_c], v after the
 * evaluations, as the protocol's transcript defines them.  Nothing is hashed here: the calls take the challenges as given.  There
 * is no blinding in these calls: kzg_circuit_quotient_blinded / kzg_circuit_open_blinded below hide the witness.  The caller's
 * term G' of kzg_circuit_quotient (gate_coset: custom gates, lookups) is NOT part of r: a circuit proved with a gate_coset cannot
 * use these calls.
 *
 * kzg_circuit_open: host pointers, synchronous, one stream slot.  wires, z and public_inputs (may be NULL) are values over H,
 * exactly as kzg_circuit_quotient takes them; t_coeffs the N - n coefficients it returned.  out_evals: 2 t x 4 u64 in the order
 * abar_0 .. abar_(t-1), sbar_0 .. sbar_(t-2), zw, each a canonical blst_fr; out_p1: the proof.  On the device: one inverse
 * transform per input column, the evaluations (the wires, PI and z from the call's coefficients, the sigmas from the circuit's
 * resident ones), then ONE launch of k_lin_combine per point: G_zeta is summed over the 3 t + e + 2 columns where they lie -- the
 * resident key, the wires, z, T -- every coefficient read once, r never written; then the scans and the MSM of kzg_open_sets.
 * Statuses, in this order: a NULL required pointer, a circuit of another context or destroyed, stride < n, a challenge not below r
 * -> KZG_ERR_INVALID_ARG; no SRS -> KZG_ERR_NO_SRS; n - 1 > kzg_srs_len -> KZG_ERR_DEGREE_TOO_HIGH; r(zeta) != 0 ->
 * KZG_ERR_REMAINDER (kzg_last_error says that the linearisation polynomial does not vanish at zeta; out_p1 is left unwritten).
 * n = 1 is legal.  Multi-device contexts as kzg_circuit_quotient: a replicated one forwards to the circuit's device, a range-split
 * one returns KZG_ERR_INVALID_ARG.  kzg_circuit_destroy waits for a running call.
 * kzg_circuit_open_device: the same on kzg_dev_alloc buffers of a single-device context (d_t_coeffs: what
 * kzg_circuit_quotient_device wrote); the evaluations and the proof come back to host memory, so only the challenges, 2 t values
 * and one point cross PCIe.
 * kzg_circuit_linearise: test hook, no SRS: the evaluations and r's n coefficients (canonical blst_fr), from the same kernel
 * launched with r's own multipliers. */
int kzg_circuit_open(kzg_ctx* ctx, const kzg_circuit* circuit, const uint64_t* wires, size_t stride, const uint64_t* z,
                     const uint64_t* public_inputs, const uint64_t* t_coeffs, const uint64_t alpha[4], const uint64_t beta[4],
                     const uint64_t gamma[4], const uint64_t zeta[4], const uint64_t v[4], uint64_t* out_evals, uint64_t out_p1[18]);
int kzg_circuit_open_device(kzg_ctx* ctx, const kzg_circuit* circuit, const void* d_wires, size_t stride, const void* d_z,
                            const void* d_public_inputs, const void* d_t_coeffs, const uint64_t alpha[4], const uint64_t beta[4],
                            const uint64_t gamma[4], const uint64_t zeta[4], const uint64_t v[4], uint64_t* out_evals,
                            uint64_t out_p1[18]);
int kzg_circuit_linearise(kzg_ctx* ctx, const kzg_circuit* circuit, const uint64_t* wires, size_t stride, const uint64_t* z,
                          const uint64_t* public_inputs, const uint64_t* t_coeffs, const uint64_t alpha[4], const uint64_t beta[4],
                          const uint64_t gamma[4], const uint64_t zeta[4], uint64_t* out_evals, uint64_t* out_r);
/* Host only, no context, like kzg_verify_sets.  key_p1s: the 2 t + 2 commitments of kzg_circuit_create, in its order; wire_p1s: the
 * t wires' commitments; t_p1s: the e - 1 commitments of T's chunks; public_inputs: n_public <= n values at rows 0 .. n_public - 1
 * (the later rows are zero; NULL for n_public = 0); evals: out_evals of the prover.  The verifier computes PI(zeta) = sum PI_i
 * L_i(zeta) with one batch inversion, forms [r] = sum scalar commitment + const G1 from the key, z_p1 and t_p1s (t + e + 3 scalar
 * multiplications, those of kzg_combine_claims) and hands the 2 t + 1 commitments and the values [0, abar, sbar, zw] to
 * kzg_verify_sets, whose setup arguments these are (one G1 entry, the G2 powers [s^j]G2 for j <= 2).  *valid = 1 accepted, 0
 * rejected.  KZG_ERR_INVALID_ARG: a NULL required pointer, a scalar not below r, a G1 input off the curve or a G2 input off the
 * twist, t outside [KZG_CIRCUIT_MIN_COLUMNS, KZG_PQ_MAX_COLUMNS], t + 1 > 2^log_ext, log_ext > KZG_PQ_MAX_LOG_EXT, n not a power
 * of two or N above 2^KZG_NTT_MAX_LOG, n_public > n. */
int kzg_circuit_verify(const uint64_t* key_p1s, size_t n, size_t t, unsigned log_ext, const uint64_t* shifts, const uint64_t* wire_p1s,
                       const uint64_t z_p1[18], const uint64_t* t_p1s, const uint64_t* public_inputs, size_t n_public,
                       const uint64_t* evals, const uint64_t alpha[4], const uint64_t beta[4], const uint64_t gamma[4],
                       const uint64_t zeta[4], const uint64_t v[4], const uint64_t proof_p1[18], const void* setup_g1,
                       size_t g1_stride_bytes, const void* setup_g2, size_t g2_stride_bytes, int* valid);

/* ---- a circuit's proof as bytes: the hashed transcript and the proof format (host only) -----------------
 * kzg_circuit_verify takes five challenges "as given".  These calls fix where they come from, so that the order -- beta and gamma
 * after the wires, alpha after [z], zeta after the [T_c], v after the evaluations -- is no longer the caller's to get wrong.
 * Hash: SHA-256.  fr(d) = the digest d read as a big-endian integer, reduced mod r (kzg_blob_challenges_bytes' reduction).
 * Scalars travel as 32 big-endian canonical bytes, points as 48 compressed bytes (kzg_g1_compress; infinity is c0 00 ..),
 * u64be(x) is 8 bytes, e = 2^log_ext:
 *     DST = ASCII "kzg_mi355x/plonk/v1"                                             (19 bytes, no terminator)
 *     h0  = SHA256(DST | u64be(n) | u64be(t) | u64be(log_ext) | u64be(n_public) | shifts (t x 32)
 *                  | key commitments ((2 t + 2) x 48, kzg_circuit_create's order) | public inputs (n_public x 32))
 *     h1  = SHA256(h0 | wire commitments (t x 48))        beta = fr(SHA256(h1 | 00)),  gamma = fr(SHA256(h1 | 01))
 *     h2  = SHA256(h1 | [z] (48))                          alpha = fr(SHA256(h2 | 00))
 *     h3  = SHA256(h2 | [T_0] .. [T_(e-2)] ((e - 1) x 48)) zeta = fr(SHA256(h3 | 00))
 *     h4  = SHA256(h3 | evaluations (2 t x 32, kzg_circuit_open's out_evals order))  v = fr(SHA256(h4 | 00))
 * PROOF BYTES, in this order: the t wire commitments, [z], the e - 1 chunk commitments, the 2 t evaluations, the opening W:
 * 48 (t + e + 1) + 64 t bytes, 576 for t = 3, e = 4 (kzg_circuit_proof_size; KZG_ERR_INVALID_ARG for a t or log_ext that
 * kzg_circuit_verify refuses).  Public inputs as for kzg_circuit_verify: n_public <= n values at rows 0 .. n_public - 1.
 * kzg_circuit_prove makes such bytes in one call; kzg_circuit_verify_proof checks them. */
int kzg_circuit_proof_size(size_t t, unsigned log_ext, size_t* bytes);
/* out: beta, gamma, alpha, zeta, v as 5 x 4 u64 (blst_fr), from complete proof bytes.  A building block and test hook: the bytes
 * are hashed as they are, no point is decoded.  KZG_ERR_INVALID_ARG: a NULL pointer (public_inputs may be NULL with n_public = 0),
 * kzg_circuit_verify's shape errors, a shift or public input not below r, proof_len other than kzg_circuit_proof_size. */
int kzg_circuit_proof_challenges(const uint64_t* key_p1s, size_t n, size_t t, unsigned log_ext, const uint64_t* shifts,
                                 const uint64_t* public_inputs, size_t n_public, const uint8_t* proof, size_t proof_len, uint64_t* out);
/* Decodes the proof, derives the challenges and calls kzg_circuit_verify.  Its argument errors are kzg_circuit_verify's, and a
 * proof_len other than kzg_circuit_proof_size is KZG_ERR_INVALID_ARG too.  A proof whose bytes do not decode -- an evaluation not
 * below r, a point kzg_g1_uncompress refuses (not on the curve, an abscissa not below p), flag bits that contradict the encoding
 * -- returns KZG_OK with *valid = 0.  Order: the pointers, the shape, proof_len, the shifts and public inputs below r and the key's
 * commitments on the curve are checked before the proof is decoded; what kzg_circuit_verify finds only in its pairing check (a
 * setup point off its curve) is reported for a proof that decodes.  Points are decoded by kzg_g1_uncompress: an on-curve check and NO subgroup check, as every
 * host verifier of this library; a caller who needs one runs kzg_g1_uncompress_batch with check_subgroup over the first
 * 48 (t + e) bytes and the last 48. */
int kzg_circuit_verify_proof(const uint64_t* key_p1s, size_t n, size_t t, unsigned log_ext, const uint64_t* shifts,
                             const uint64_t* public_inputs, size_t n_public, const uint8_t* proof, size_t proof_len, const void* setup_g1,
                             size_t g1_stride_bytes, const void* setup_g2, size_t g2_stride_bytes, int* valid);

/* The proof of a circuit in one call: the five rounds under the transcript above, every challenge derived inside.
 *   1. the wires go to the device and to coefficient form (with their blinder patches when blinded), are committed; beta, gamma
 *   2. z is formed on the device from the wires and the circuit's resident sigma values (kzg_permutation_product_device's work,
 *      nothing downloaded); z_n != 1 -> KZG_ERR_REMAINDER; z is committed; alpha
 *   3. the quotient and its chunks' commitments; zeta          4. the evaluations; v, which is fixed AFTER them
 *   5. r, r(zeta) = 0 tested before the MSM, the opening W
 * key_p1s: the (2 t + 2) x 18 commitments of kzg_circuit_create (they enter the transcript).  wires: t columns of n blst_fr, column j
 * at wires + 4 j stride u64.  public_inputs: n_public <= n values at rows 0 .. n_public - 1 (NULL with n_public = 0); they are
 * padded with zeros to n values and added "as given", as kzg_circuit_quotient does.  blinders: NULL for a plain proof, which is
 * NOT zero-knowledge, else kzg_circuit_blinders' array.  out_proof: kzg_circuit_proof_size bytes.
 * The bytes are bit for bit what the existing calls give when chained by hand with the transcript's challenges: blinded
 * kzg_commit_evaluations_blinded (wires with nb = 2, z with nb = 3), kzg_circuit_quotient_blinded, kzg_circuit_open_blinded; plain
 * kzg_commit_evaluations, kzg_circuit_quotient, kzg_circuit_open; the outputs compressed and serialised.
 * The call holds one slot and takes its turn with the quotient calls from start to end.  Every per-proof column is transformed
 * back ONCE (the hand chain does it three times), the transforms of more than one column are batched (k_nttb_pass), and nothing
 * but the wires, the public inputs, the blinders and the proof crosses PCIe apart from what the rounds exchange anyway: the
 * commitments off the MSM's host tail, the 2 t + 1 evaluation words and r(zeta).
 * MEMORY: what lives across the rounds -- the values and the coefficients of the t + 2 per-proof columns, the blinded copies, T --
 * sits in device buffers that the context keeps after the first proof, grown to the largest proof made and freed only by
 * kzg_ctx_destroy: about (3 t + e + 5) n x 32 bytes for a blinded proof with public inputs, 544 MiB at n = 2^20, t = 3, e = 4.
 * HOST TIME: the transcript hashes every public input, so a proof (and kzg_circuit_verify_proof) with n_public = 2^20 spends 55 ms
 * of host time on them alone; with the few public inputs a statement usually has it is microseconds.
 * Statuses, in this order: KZG_ERR_INVALID_ARG (NULL pointers, a circuit of another context, stride < n, n_public > n, a public
 * input or blinder not below r, for blinded proofs the shape rule N >= t n + t + 4), KZG_ERR_NO_SRS, KZG_ERR_DEGREE_TOO_HIGH (n
 * points for a plain proof, n + t + 3 for a blinded one), the grand product's zero-denominator status with its message,
 * KZG_ERR_REMAINDER (z_n != 1, the quotient, r(zeta)).  A failed call writes nothing to out_proof and leaves the context serving.
 * Multi-device contexts as kzg_circuit_quotient with commitments: a replicated one forwards, a range-split one is refused. */
int kzg_circuit_prove(kzg_ctx* ctx, const kzg_circuit* circuit, const uint64_t* key_p1s, const uint64_t* wires, size_t stride,
                      const uint64_t* public_inputs, size_t n_public, const uint64_t* blinders, uint8_t* out_proof);
/* the same with the wires in a kzg_dev_alloc buffer of a single-device context (public inputs, blinders and the proof stay host) */
int kzg_circuit_prove_device(kzg_ctx* ctx, const kzg_circuit* circuit, const uint64_t* key_p1s, const void* d_wires, size_t stride,
                             const uint64_t* public_inputs, size_t n_public, const uint64_t* blinders, uint8_t* out_proof);

/* ---- a circuit with a lookup table: the LogUp term of the quotient -------------------------------------
 * Notation as in the sections above.  A lookup circuit keeps, beside the 2 t + 2 columns of kzg_circuit_create, c table columns
 * tab_0 .. tab_(c-1) (1 <= c <= t, n values each) and one lookup selector q_K.  STATEMENT: for every row i the tuple
 * q_K[i] (f_0[i], .., f_(c-1)[i]) is a row of the table.  A row with q_K = 0 looks up the zero tuple, which the table must then
 * hold: that is the circuit author's obligation.  With challenges theta and beta:
 *     F(X) = beta + q_K(X) sum_(j<c) theta^j f_j(X)         Tt(X) = beta + sum_(j<c) theta^j tab_j(X)
 *     f_i = F_i - beta, T_i = Tt_i - beta over H;  m = the multiplicities of the column f in the column T by
 *         kzg_lookup_multiplicities' rule (k = 1, n_table = n: the count sits at the LEAST row holding the value)
 *     phi_0 = 0, phi_(i+1) = phi_i + 1 / (beta + f_i) - m_i / (beta + T_i)   (kzg_lookup_sum, k = 1); phi_n must be 0
 *     Lk1 = (phi(w X) - phi(X)) F Tt - Tt + m F             Lk2 = L_0 phi
 *     G'  = alpha^3 Lk1 + alpha^4 Lk2,   Num_L = Num (of kzg_circuit_quotient, no caller's term) + G',   T = Num_L / (X^n - 1).
 * deg G' = 4 (n - 1), hence the shape rules e >= max(t + 1, 4) and 3 t + e + c + 5 <= 32 (the columns a last round combines at
 * zeta).  These calls are the pieces of a proof; nothing in them is blinded, so what is built from them is NOT zero-knowledge.
 *
 * kzg_circuit_create_lookup is kzg_circuit_create with the table (c columns of n values, column j at table + 4 j table_stride u64)
 * and q_lookup (n values): the c + 1 columns are resident as values, coefficients and coset values behind the others, in the
 * order tab_0 .. tab_(c-1), q_K, and out_key_p1s (NULL, or (2 t + c + 3) x 18 u64) receives kzg_circuit_create's commitments and
 * then theirs, each bit for bit kzg_commit_evaluations of the column.  Device memory: kzg_circuit_create's with 2 t + c + 3 columns
 * in place of 2 t + 2.  Every call that takes a circuit accepts the handle and ignores the table.  KZG_ERR_INVALID_ARG:
 * kzg_circuit_create's rules, c < 1, c > t, 2^log_ext < 4, 3 t + 2^log_ext + c + 5 > 32, table_stride < n, a NULL table or q_lookup.
 * kzg_circuit_column_device hands the columns out as KZG_CIRCUIT_COL_TABLE + j (j < c) and KZG_CIRCUIT_COL_QLOOKUP; on a circuit
 * without a table these are KZG_ERR_INVALID_ARG.
 *
 * kzg_circuit_lookup_columns computes the per-proof columns on the device: wires as kzg_circuit_quotient takes them (the first c
 * columns are read) -> out_f and out_table (NULL, or n x 4 u64: the folded columns f and T), out_mult (m), out_phi (phi_0 ..
 * phi_(n-1)) and out_last (phi_n), canonical blst_fr.  Needs no SRS.  KZG_ERR_INVALID_ARG with *bad_row (may be NULL) = the least
 * row when a folded tuple is in no table row or a denominator beta + f_i, beta + T_i is zero, with kzg_lookup_multiplicities' and
 * kzg_lookup_sum's messages; else *bad_row = (size_t)-1.  Also KZG_ERR_INVALID_ARG: a NULL required pointer, a circuit without a
 * table or of another context, stride < n.  On a multi-device context the call runs on devices[0].
 *
 * kzg_circuit_lookup_quotient is kzg_circuit_quotient with the lookup's term in place of the caller's: mult and phi (n values
 * each, as kzg_circuit_lookup_columns returned them) are extended with the wires, G' is computed on the coset, and T, its
 * outputs, statuses and multi-device rules are kzg_circuit_quotient's.  beta is the lookup's beta and the permutation's.
 * KZG_ERR_REMAINDER also when m or phi are not those of the wires, or phi_n != 0.
 *
 * THE PROOF.  Last round: with the new evaluations tbar_j = tab_j(zeta), qbar = q_K(zeta), phiw = phi(zeta w), Fbar = beta + qbar
 * sum_j theta^j abar_j, Tbar = beta + sum_j theta^j tbar_j, l = L_0(zeta) and r the polynomial of kzg_circuit_open formed with this T,
 *     r_L(X) = r(X) + (alpha^4 l - alpha^3 Fbar Tbar) phi(X) + alpha^3 Fbar m(X) + alpha^3 (phiw Fbar Tbar - Tbar),
 * and the opening is kzg_open_sets over the 2 t + c + 3 polynomials
 *     [ r_L | f_0 .. f_(t-1) | sigma_0 .. sigma_(t-2) | z | tab_0 .. tab_(c-1) | q_K | phi ],
 * z and phi in the set {zeta w}, the rest in {zeta}, gamma := v.  Transcript: SHA-256 with the encodings of kzg_circuit_prove and a
 * domain of its own, so that no plain proof parses as a lookup proof:
 *     DST = ASCII "kzg_mi355x/plonk-lookup/v1"
 *     h0 = SHA256(DST | u64be(n) | u64be(t) | u64be(log_ext) | u64be(c) | u64be(n_public) | shifts (t x 32)
 *                 | key commitments ((2 t + c + 3) x 48, kzg_circuit_create_lookup's order) | public inputs)
 *     h1 = SHA256(h0 | wire commitments)     theta = fr(SHA256(h1 | 00))
 *     h2 = SHA256(h1 | [m])                  beta = fr(SHA256(h2 | 00)), gamma = fr(SHA256(h2 | 01))
 *     h3 = SHA256(h2 | [z] | [phi])          alpha = fr(SHA256(h3 | 00))
 *     h4 = SHA256(h3 | [T_0] .. [T_(e-2)])   zeta = fr(SHA256(h4 | 00))
 *     h5 = SHA256(h4 | evaluations)          v = fr(SHA256(h5 | 00))
 * Proof bytes, in order: the t wire commitments, [m], [z], [phi], the e - 1 chunk commitments (48 bytes each), the 2 t + c + 2
 * evaluations abar_0.., sbar_0 .. sbar_(t-2), z(zeta w), tbar_0.., qbar, phiw (32 bytes each), W: 48 (t + e + 3) + 32 (2 t + c + 2)
 * bytes (kzg_circuit_lookup_proof_size), 832 at t = 3, e = 4, c = 3.  Every commitment is bit for bit kzg_commit_evaluations of its
 * column.  Proofs of kzg_circuit_lookup_prove are plain; the _blinded forms are zero-knowledge: in a plain proof neither the wires
 * nor z, phi, m or T are blinded, so it is NOT zero-knowledge.
 *
 * kzg_circuit_lookup_prove: host wires, synchronous, one stream slot; key_p1s the (2 t + c + 3) x 18 u64 of
 * kzg_circuit_create_lookup; public_inputs the first n_public values of PI (the rest zero), or NULL with n_public = 0; out_proof
 * receives kzg_circuit_lookup_proof_size bytes.  Rounds: the wires, then theta; the folded columns, the multiplicities, [m], then
 * beta and gamma; phi and z, both committed, then alpha; the quotient; the opening.  Statuses, in this order:
 * KZG_ERR_INVALID_ARG (a NULL required pointer, a circuit without a table or of another context, stride < n, n_public > n, a public
 * input not below r); KZG_ERR_NO_SRS; KZG_ERR_DEGREE_TOO_HIGH (the SRS has fewer than n points); KZG_ERR_REMAINDER with *bad_row
 * (may be NULL) = the least row whose tuple is not in the table, and kzg_last_error naming the row; the running sum's status for
 * a zero denominator (KZG_ERR_INVALID_ARG, its message, *bad_row the row); KZG_ERR_REMAINDER for z_n != 1, phi_n != 0, a quotient
 * that leaves a remainder, or r_L(zeta) != 0.  Else *bad_row = (size_t)-1.  A failed call writes nothing to out_proof and leaves the
 * context serving.  Multi-device rules are kzg_circuit_prove's.  The _device form takes the wires in a kzg_dev_alloc buffer of a
 * single-device context.
 *
 * Host only, no context: kzg_circuit_lookup_proof_size; kzg_circuit_lookup_proof_challenges (out: 6 x 4 u64, theta, beta, gamma,
 * alpha, zeta, v as blst_fr, from complete proof bytes; nothing is decoded); kzg_circuit_lookup_verify_proof, whose argument and
 * decode rules are kzg_circuit_verify_proof's: bytes that do not decode give KZG_OK with *valid = 0, there is no subgroup check.
 * [r_L] is formed from the key, [z], [m], [phi] and the [T_c] and handed to kzg_verify_sets.
 *
 * THE BLINDED FORMS make the lookup proof zero-knowledge; the verifier, the proof's format and size and the
 * transcript do not change.  With Z_H = X^n - 1 the wires, z and T's chunks are blinded as in kzg_circuit_prove, and
 *     phi~ = phi + (p_0 + p_1 X + p_2 X^2) Z_H   (linearised at zeta and opened at zeta w, like z: three blinders)
 *     m~   = m + (u_0 + u_1 X) Z_H               (committed once, enters through r_L at zeta only: two blinders)
 * T~ = Num_L(f~, z~, phi~, m~) / Z_H has D = max(t n + t + 3, 3 n + 2) coefficients and is returned as L_T = (e - 1) n + t + 3,
 * zeros from D on.  Shape rule: kzg_circuit_create_lookup's, D < N and D <= L_T.  The blinder array is kzg_circuit_prove's (t pairs,
 * c_0..c_2, d_0..d_(e-3)) with p_0, p_1, p_2 and then u_0, u_1 behind it: 2 t + e + 6 canonical blst_fr.  The SRS needs n + t + 3
 * points.  With every blinder zero the proof is kzg_circuit_lookup_prove's, byte for byte.
 * kzg_circuit_lookup_blinded_sizes (host only) applies the shape rule (KZG_ERR_INVALID_ARG for a refused shape) -> the entries of
 * the array and L_T.  kzg_circuit_lookup_blinders draws the array from the OS CSPRNG, as kzg_circuit_blinders does.
 * kzg_circuit_lookup_quotient_blinded is kzg_circuit_lookup_quotient for the blinded columns: out_coeffs (NULL, or L_T x 4 u64)
 * and out_p1s (NULL, or the (e - 1) commitments of the blinded chunks T~_c, n + t + 3 SRS points); statuses are
 * kzg_circuit_lookup_quotient's in their order, the shape rule and then a blinder not below r (KZG_ERR_INVALID_ARG) behind the
 * circuit's checks.  kzg_circuit_lookup_prove_blinded / _device are kzg_circuit_lookup_prove / _device with blinders (required):
 * the same rounds and transcript, [m~] and [phi~] committed from n + 2 and n + 3 coefficients; statuses are
 * kzg_circuit_lookup_prove's in their order, *bad_row included, with the shape rule and a blinder not below r right behind the
 * argument checks and KZG_ERR_DEGREE_TOO_HIGH for an SRS of fewer than n + t + 3 points.  A failed call writes nothing to out_proof
 * and leaves the context serving.  Multi-device rules are kzg_circuit_prove's. */
int kzg_circuit_lookup_blinded_sizes(size_t n, size_t t, unsigned log_ext, size_t c, size_t* num_blinders, size_t* quotient_len);
int kzg_circuit_lookup_blinders(size_t t, unsigned log_ext, uint64_t* out /* (2t+e+6)x4 */);
int kzg_circuit_lookup_quotient_blinded(kzg_ctx* ctx, const kzg_circuit* circuit, const uint64_t* wires, size_t stride,
                                        const uint64_t* z, const uint64_t* mult, const uint64_t* phi, const uint64_t* public_inputs,
                                        const uint64_t alpha[4], const uint64_t beta[4], const uint64_t gamma[4],
                                        const uint64_t theta[4], const uint64_t* blinders, uint64_t* out_coeffs /* L_T x 4 */,
                                        uint64_t* out_p1s /* (e-1) x 18 */);
int kzg_circuit_lookup_prove_blinded(kzg_ctx* ctx, const kzg_circuit* circuit, const uint64_t* key_p1s, const uint64_t* wires,
                                     size_t stride, const uint64_t* public_inputs, size_t n_public, const uint64_t* blinders,
                                     uint8_t* out_proof, size_t* bad_row);
int kzg_circuit_lookup_prove_blinded_device(kzg_ctx* ctx, const kzg_circuit* circuit, const uint64_t* key_p1s, const void* d_wires,
                                            size_t stride, const uint64_t* public_inputs, size_t n_public, const uint64_t* blinders,
                                            uint8_t* out_proof, size_t* bad_row);
int kzg_circuit_lookup_prove(kzg_ctx* ctx, const kzg_circuit* circuit, const uint64_t* key_p1s, const uint64_t* wires, size_t stride,
                             const uint64_t* public_inputs, size_t n_public, uint8_t* out_proof, size_t* bad_row);
int kzg_circuit_lookup_prove_device(kzg_ctx* ctx, const kzg_circuit* circuit, const uint64_t* key_p1s, const void* d_wires,
                                    size_t stride, const uint64_t* public_inputs, size_t n_public, uint8_t* out_proof,
                                    size_t* bad_row);
int kzg_circuit_lookup_proof_size(size_t t, unsigned log_ext, size_t c, size_t* bytes);
int kzg_circuit_lookup_proof_challenges(const uint64_t* key_p1s, size_t n, size_t t, unsigned log_ext, size_t c,
                                        const uint64_t* shifts, const uint64_t* public_inputs, size_t n_public, const uint8_t* proof,
                                        size_t proof_len, uint64_t* out);
int kzg_circuit_lookup_verify_proof(const uint64_t* key_p1s, size_t n, size_t t, unsigned log_ext, size_t c, const uint64_t* shifts,
                                    const uint64_t* public_inputs, size_t n_public, const uint8_t* proof, size_t proof_len,
                                    const void* setup_g1, size_t g1_stride_bytes, const void* setup_g2, size_t g2_stride_bytes,
                                    int* valid);
#define KZG_CIRCUIT_COL_TABLE 64
#define KZG_CIRCUIT_COL_QLOOKUP 80
int kzg_circuit_create_lookup(kzg_ctx* ctx, const uint64_t* q_lin, const uint64_t* q_mul, const uint64_t* q_const,
                              const uint64_t* sigmas, size_t n, size_t t, size_t stride, const uint64_t* shifts, unsigned log_ext,
                              const uint64_t* table, size_t c, size_t table_stride, const uint64_t* q_lookup,
                              uint64_t* out_key_p1s /* (2t+c+3)x18 */, kzg_circuit** out);
int kzg_circuit_lookup_columns(kzg_ctx* ctx, const kzg_circuit* circuit, const uint64_t* wires, size_t stride, const uint64_t theta[4],
                               const uint64_t beta[4], uint64_t* out_f, uint64_t* out_table, uint64_t* out_mult, uint64_t* out_phi,
                               uint64_t out_last[4], size_t* bad_row);
int kzg_circuit_lookup_quotient(kzg_ctx* ctx, const kzg_circuit* circuit, const uint64_t* wires, size_t stride, const uint64_t* z,
                                const uint64_t* mult, const uint64_t* phi, const uint64_t* public_inputs, const uint64_t alpha[4],
                                const uint64_t beta[4], const uint64_t gamma[4], const uint64_t theta[4], uint64_t* out_coeffs,
                                uint64_t* out_p1s);

/* ---- circuit proofs with custom gates: selector x wire-monomial terms ----------------------------------
 * Notation as above.  A custom circuit keeps g more resident selector columns qx_0 .. qx_(g-1) (n values each) and an exponent
 * matrix p[s][j] in 0..7 (g x t bytes, row-major), d_s = sum_j p[s][j], d_max = max_s d_s.  Every row i must satisfy
 *     sum_j q_j f_j + q_M f_0 f_1 + q_C + PI + sum_(s<g) qx_s[i] prod_(j<t) f_j[i]^p[s][j] = 0
 *     G'(X) = sum_s qx_s(X) prod_j f_j(X)^p[s][j],   Num_X = Num (of kzg_circuit_quotient, no caller's term) + G',
 *     T = Num_X / (X^n - 1);   deg G' <= (d_max + 1)(n - 1), so T's share has degree below d_max n.
 * Shape rules (KZG_ERR_INVALID_ARG from kzg_circuit_create_custom): kzg_circuit_create's, 1 <= g <= KZG_CIRCUIT_MAX_CUSTOM, an
 * exponent above 7, a term of degree d_s = 0 (that is q_C), 2^log_ext < max(t + 1, d_max + 1), 3 t + 2^log_ext + 3 + g > 32 (the
 * columns the last round combines at zeta), custom_stride < n, a NULL q_custom or exponents.  Terms at the next row
 * f_j(w X) are the next section's.  Not offered: a custom circuit with a lookup table, a caller's gate_coset on top of the custom terms.
 *
 * kzg_circuit_create_custom is kzg_circuit_create with q_custom (g columns of n values, column s at q_custom + 4 s custom_stride
 * u64) and exponents: the g columns are resident as values, coefficients and coset values behind the 2 t + 2 others and
 * out_key_p1s (NULL, or (2 t + 2 + g) x 18 u64) receives kzg_circuit_create's commitments and then theirs, each bit for bit
 * kzg_commit_evaluations of the column.  Device memory: kzg_circuit_create's with 2 t + 2 + g columns.  Every other call that takes
 * a circuit accepts the handle and ignores the custom terms (kzg_circuit_prove proves the base statement).
 * kzg_circuit_column_device hands the columns out as KZG_CIRCUIT_COL_CUSTOM + s (s < g).
 *
 * kzg_circuit_custom_gate (the kernel's test hook): wires as kzg_circuit_quotient takes them -> out_gate_coset, the N values
 * G'(x_i) on the coset of kzg_circuit_quotient's gate_coset, canonical blst_fr.  Needs no SRS; a multi-device context runs it on
 * devices[0].  kzg_circuit_custom_quotient is kzg_circuit_quotient (blinders NULL; out_coeffs N - n values) or
 * kzg_circuit_quotient_blinded (out_coeffs L_T values) with G' as the caller's term, computed on the device from the (blinded)
 * wires; outputs, statuses and multi-device rules are theirs.  An unsatisfied custom gate is KZG_ERR_REMAINDER.
 *
 * BLINDING is kzg_circuit_prove's: the array, the wires, z and T's chunks as in the section above; the selectors are key material
 * and are not blinded.  Only T~'s degree changes: deg T~ = max(t n + t + 2, d_max (n + 1) - 1), and a blinded call is
 * KZG_ERR_INVALID_ARG unless deg T~ + 1 <= L_T = (e - 1) n + t + 3 and N >= deg T~ + 2 (for d_max <= t the rule above, unchanged).
 * kzg_circuit_custom_blinded_sizes (host only) applies the rule; its outputs are kzg_circuit_blinded_sizes'.
 *
 * THE PROOF.  Last round: r_X(X) = r(X) + sum_s (prod_j abar_j^p[s][j]) qx_s(X) with r the polynomial of kzg_circuit_open formed with
 * this T; the opening stack, the 2 t evaluations and the sets are the plain proof's.  Proof bytes: kzg_circuit_prove's format and
 * kzg_circuit_proof_size(t, log_ext) bytes; every commitment is bit for bit kzg_commit_evaluations (blinded:
 * kzg_commit_evaluations_blinded) of its column.  Transcript: kzg_circuit_prove's from h1 on under a statement of its own, so that no
 * plain proof verifies as a custom proof of the same key prefix:
 *     DST = ASCII "kzg_mi355x/plonk-custom/v1"
 *     h0 = SHA256(DST | u64be(n) | u64be(t) | u64be(log_ext) | u64be(g) | u64be(n_public) | shifts (t x 32)
 *                 | exponents (g x t bytes, row-major) | key commitments ((2 t + 2 + g) x 48, kzg_circuit_create_custom's order)
 *                 | public inputs)
 * kzg_circuit_custom_prove / _device: kzg_circuit_prove's arguments (key_p1s: (2 t + 2 + g) x 18 u64; blinders NULL for a plain
 * proof), statuses in kzg_circuit_prove's order, with KZG_ERR_INVALID_ARG also for a circuit without custom gates and for the
 * blinded rule, and KZG_ERR_REMAINDER from the quotient for an unsatisfied custom gate or from r_X(zeta) != 0.  A failed call writes
 * nothing to out_proof and leaves the context serving.  Multi-device rules are kzg_circuit_prove's.
 *
 * Host only, no context: kzg_circuit_custom_proof_challenges (out: 5 x 4 u64, beta, gamma, alpha, zeta, v as
 * kzg_circuit_proof_challenges) and kzg_circuit_custom_verify_proof, which adds sum_s (prod_j abar_j^p[s][j]) [qx_s] to [r] and runs
 * kzg_verify_sets; argument and decode rules are kzg_circuit_verify_proof's plus the shape rules above: bytes that do not decode
 * give KZG_OK with *valid = 0.  The verifier is the same for plain and blinded proofs. */
#define KZG_CIRCUIT_MAX_CUSTOM 8
#define KZG_CIRCUIT_COL_CUSTOM 96
int kzg_circuit_create_custom(kzg_ctx* ctx, const uint64_t* q_lin, const uint64_t* q_mul, const uint64_t* q_const,
                              const uint64_t* sigmas, size_t n, size_t t, size_t stride, const uint64_t* shifts, unsigned log_ext,
                              const uint64_t* q_custom, size_t g, size_t custom_stride, const uint8_t* exponents /* g*t */,
                              uint64_t* out_key_p1s /* (2t+2+g)x18 */, kzg_circuit** out);
int kzg_circuit_custom_gate(kzg_ctx* ctx, const kzg_circuit* circuit, const uint64_t* wires, size_t stride,
                            uint64_t* out_gate_coset /* N x 4 */);
int kzg_circuit_custom_quotient(kzg_ctx* ctx, const kzg_circuit* circuit, const uint64_t* wires, size_t stride, const uint64_t* z,
                                const uint64_t* public_inputs, const uint64_t alpha[4], const uint64_t beta[4], const uint64_t gamma[4],
                                const uint64_t* blinders /* NULL: plain */, uint64_t* out_coeffs, uint64_t* out_p1s);
int kzg_circuit_custom_prove(kzg_ctx* ctx, const kzg_circuit* circuit, const uint64_t* key_p1s, const uint64_t* wires, size_t stride,
                             const uint64_t* public_inputs, size_t n_public, const uint64_t* blinders, uint8_t* out_proof);
int kzg_circuit_custom_prove_device(kzg_ctx* ctx, const kzg_circuit* circuit, const uint64_t* key_p1s, const void* d_wires,
                                    size_t stride, const uint64_t* public_inputs, size_t n_public, const uint64_t* blinders,
                                    uint8_t* out_proof);
int kzg_circuit_custom_proof_challenges(const uint64_t* key_p1s, size_t n, size_t t, unsigned log_ext, size_t g,
                                        const uint8_t* exponents, const uint64_t* shifts, const uint64_t* public_inputs, size_t n_public,
                                        const uint8_t* proof, size_t proof_len, uint64_t* out);
int kzg_circuit_custom_verify_proof(const uint64_t* key_p1s, size_t n, size_t t, unsigned log_ext, size_t g, const uint8_t* exponents,
                                    const uint64_t* shifts, const uint64_t* public_inputs, size_t n_public, const uint8_t* proof,
                                    size_t proof_len, const void* setup_g1, size_t g1_stride_bytes, const void* setup_g2,
                                    size_t g2_stride_bytes, int* valid);
int kzg_circuit_custom_blinded_sizes(size_t n, size_t t, unsigned log_ext, size_t d_max, size_t* num_blinders, size_t* quotient_len);

/* ---- custom gates that read the next row: f_j(w X) terms -------------------------------------------------
 * A next-row circuit is a custom circuit of the section above with a second exponent matrix p'[s][j] in 0..7 (g x t bytes, row-major,
 * like p).  Every row i, with i + 1 taken mod n, must satisfy
 *     sum_j q_j f_j + q_M f_0 f_1 + q_C + PI + sum_(s<g) qx_s[i] prod_j f_j[i]^p[s][j] prod_j f_j[i+1]^p'[s][j] = 0
 *     G'(X) = sum_s qx_s(X) prod_j f_j(X)^p[s][j] prod_j f_j(w X)^p'[s][j]
 * with d_s = sum_j (p[s][j] + p'[s][j]), d_max = max_s d_s, R = { j : some p'[s][j] > 0 } ascending and rho = |R|.  deg G' <=
 * (d_max + 1)(n - 1) as before: T's chunks and the plain degree rule do not change.  On the coset f_j(w x_i) is the extended wire
 * column at index (i + e) mod N, e = 2^log_ext: no new transform, one kernel (k_cgn_gate).
 * Shape rules (KZG_ERR_INVALID_ARG from kzg_circuit_create_custom_next and again from the verifier): kzg_circuit_create_custom's with
 * the d_s above (1 <= g <= 8, exponents <= 7, d_s >= 1, 2^log_ext >= max(t + 1, d_max + 1), 3 t + 2^log_ext + 3 + g <= 32), rho >= 1
 * (a circuit with no next-row exponent is kzg_circuit_create_custom's), n >= 2 (at n = 1, w = 1 and {zeta, zeta w} would hold one
 * point twice), a NULL exponents_next.
 *
 * kzg_circuit_create_custom_next is kzg_circuit_create_custom with exponents_next: the same resident columns, the same out_key_p1s
 * of (2 t + 2 + g) x 18 u64.  kzg_circuit_custom_next_gate (the kernel's test hook, no SRS) and kzg_circuit_custom_next_quotient
 * (the plain quotient: out_coeffs N - n values, out_p1s 2^log_ext - 1 commitments) are kzg_circuit_custom_gate and
 * kzg_circuit_custom_quotient with blinders NULL, with G' as above.  A kzg_circuit_custom_* call on a next-row handle is
 * KZG_ERR_INVALID_ARG (ignoring p' would prove a different statement), and so is a kzg_circuit_custom_next_* call on a custom handle
 * without p'; the plain calls (kzg_circuit_prove, ...) accept the handle and ignore all custom terms.
 *
 * THE PROOF.  With abar_j = f_j(zeta) and abar'_j = f_j(zeta w) for j in R:
 *     r_N(X) = r(X) + sum_s (prod_j abar_j^p[s][j] prod_j abar'_j^p'[s][j]) qx_s(X)
 * The stack stays [ r_N | f_0 .. f_(t-1) | sigma_0 .. sigma_(t-2) | z ] on three sets over the same two points: S_0 = {zeta} (r_N, the
 * wires outside R, the sigmas), S_1 = {zeta w} (z), S_2 = {zeta, zeta w} (the wires in R).  The proof element is bit for bit
 * kzg_open_sets of that stack on those sets with gamma = v.  Proof bytes: t + 2^log_ext + 1 compressed points in the plain format's
 * places and 2 t + rho big-endian scalars where it has 2 t: the plain format's, then abar'_j for j in R ascending;
 * kzg_circuit_custom_next_proof_size(t, log_ext, rho) = 48 (t + 2^log_ext + 1) + 32 (2 t + rho).  Transcript: kzg_circuit_prove's
 * from h1 on, v drawn after all 2 t + rho evaluations, under a statement of its own, so that no custom proof verifies as a next-row
 * proof of the same key and p, nor the reverse:
 *     DST = ASCII "kzg_mi355x/plonk-custom-next/v1"
 *     h0 = SHA256(DST | u64be(n) | u64be(t) | u64be(log_ext) | u64be(g) | u64be(n_public) | shifts (t x 32) | exponents (g x t)
 *                 | next-row exponents (g x t) | key commitments ((2 t + 2 + g) x 48) | public inputs)
 * kzg_circuit_custom_next_prove / _device: kzg_circuit_custom_prove's arguments, statuses and multi-device rules.  NEXT-ROW PROOFS ARE
 * PLAIN, NOT ZERO-KNOWLEDGE: a wire opened at two points needs a third blinder, which changes the blinder array, the patch kernels'
 * counts and the degree rule; blinders != NULL is KZG_ERR_INVALID_ARG.  KZG_ERR_REMAINDER from the quotient for an unsatisfied term
 * (the term of row n - 1 reads row 0) or from r_N(zeta) != 0; a failed call writes nothing to out_proof and leaves the context serving.
 * Host only, no context: kzg_circuit_custom_next_proof_size, kzg_circuit_custom_next_proof_challenges (out: 5 x 4 u64 as
 * kzg_circuit_proof_challenges) and kzg_circuit_custom_next_verify_proof, which rebuilds [r_N] from the key and runs kzg_verify_sets
 * over the three sets (setup_g1: [s^j]G1 for j < 2, the largest set has two points; setup_g2: [s^j]G2 for j <= 2); bytes that do not
 * decode give KZG_OK with *valid = 0.
 * Not offered: blinding, rows further than i + 1, a lookup table beside the terms, submit / wait forms. */
int kzg_circuit_create_custom_next(kzg_ctx* ctx, const uint64_t* q_lin, const uint64_t* q_mul, const uint64_t* q_const,
                                   const uint64_t* sigmas, size_t n, size_t t, size_t stride, const uint64_t* shifts, unsigned log_ext,
                                   const uint64_t* q_custom, size_t g, size_t custom_stride, const uint8_t* exponents /* g*t */,
                                   const uint8_t* exponents_next /* g*t */, uint64_t* out_key_p1s /* (2t+2+g)x18 */, kzg_circuit** out);
int kzg_circuit_custom_next_gate(kzg_ctx* ctx, const kzg_circuit* circuit, const uint64_t* wires, size_t stride,
                                 uint64_t* out_gate_coset /* N x 4 */);
int kzg_circuit_custom_next_quotient(kzg_ctx* ctx, const kzg_circuit* circuit, const uint64_t* wires, size_t stride, const uint64_t* z,
                                     const uint64_t* public_inputs, const uint64_t alpha[4], const uint64_t beta[4],
                                     const uint64_t gamma[4], uint64_t* out_coeffs, uint64_t* out_p1s);
int kzg_circuit_custom_next_prove(kzg_ctx* ctx, const kzg_circuit* circuit, const uint64_t* key_p1s, const uint64_t* wires, size_t stride,
                                  const uint64_t* public_inputs, size_t n_public, const uint64_t* blinders /* NULL */,
                                  uint8_t* out_proof);
int kzg_circuit_custom_next_prove_device(kzg_ctx* ctx, const kzg_circuit* circuit, const uint64_t* key_p1s, const void* d_wires,
                                         size_t stride, const uint64_t* public_inputs, size_t n_public,
                                         const uint64_t* blinders /* NULL */, uint8_t* out_proof);
int kzg_circuit_custom_next_proof_size(size_t t, unsigned log_ext, size_t rho, size_t* bytes);
int kzg_circuit_custom_next_proof_challenges(const uint64_t* key_p1s, size_t n, size_t t, unsigned log_ext, size_t g,
                                             const uint8_t* exponents, const uint8_t* exponents_next, const uint64_t* shifts,
                                             const uint64_t* public_inputs, size_t n_public, const uint8_t* proof, size_t proof_len,
                                             uint64_t* out);
int kzg_circuit_custom_next_verify_proof(const uint64_t* key_p1s, size_t n, size_t t, unsigned log_ext, size_t g, const uint8_t* exponents,
                                         const uint8_t* exponents_next, const uint64_t* shifts, const uint64_t* public_inputs,
                                         size_t n_public, const uint8_t* proof, size_t proof_len, const void* setup_g1,
                                         size_t g1_stride_bytes, const void* setup_g2, size_t g2_stride_bytes, int* valid);

/* ---- many proofs of one key with one pairing check ------------------------------------------------------
 * kzg_circuit_verify_proofs_batch: proof k (k < count) is at proofs + k proof_len, its public inputs (n_public blst_fr) at
 * public_inputs + 4 k pi_stride; every proof is claimed for the one key key_p1s.  g = 0 with exponents NULL is the plain
 * statement (kzg_mi355x/plonk/v1, kzg_circuit_verify_proof's), g >= 1 the custom statement (kzg_mi355x/plonk-custom/v1) with
 * kzg_circuit_custom_verify_proof's key of 2 t + 2 + g commitments and its g x t exponents; both share one proof format.
 * With A_0k = sum_(i < 2t) v^i C_i - [sum v^i y_i]G1 and A_1k = v^(2t) [z] - [v^(2t) z(zeta w)]G1 of proof k as kzg_verify_sets
 * forms them from kzg_circuit_verify's stack, and weights rho_k = a_k + b_k lambda (a_k, b_k uniform 64-bit from getrandom(2),
 * fresh on every call), the device forms
 *     P0 = sum_k rho_k (-zeta_k w A_0k - zeta_k A_1k - zeta_k^2 w W_k)
 *     P1 = sum_k rho_k (A_0k + A_1k + zeta_k (1 + w) W_k)
 *     P2 = -sum_k rho_k W_k
 * and the host pairs once: e(P0, [1]G2) e(P1, [s]G2) e(P2, [s^2]G2) == 1, three pairs and one final exponentiation whatever
 * count is.  *valid = 1 when every proof is valid; a batch holding an invalid proof is accepted with probability at most 2^-128;
 * count = 0 gives *valid = 1.  setup_g2 is read at indices 0, 1 and 2 as kzg_circuit_verify reads it; [1]G1 is the context's
 * SRS[0].  The host hashes the transcripts (at most 16 threads), draws the weights and pairs; the decoding of the points and the
 * evaluations, PI(zeta_k), the scalars, every scalar multiplication and the sums run on the device: about t + e + 6 ladders per
 * proof and 2 (2 t + 3 + g) for the key.
 * A proof whose bytes do not decode (a point, or an evaluation not below r) or with a point outside G1 (the order-r subgroup)
 * is invalid, not an error: KZG_OK, *valid = 0 and *bad_index (may be NULL) the least such proof.  THIS IS STRICTER THAN
 * kzg_circuit_verify_proof, which checks the curve equation only: the endomorphism the device's ladders use acts as lambda
 * only on G1, so a point outside it cannot be multiplied and is refused.  When every proof decodes and only the pairing fails,
 * *bad_index = SIZE_MAX: the call does not locate the proof; bisect, or fall back to kzg_circuit_verify_proof.
 * Errors, checked in this order, *valid untouched (kzg_last_error names the proof):
 *   KZG_ERR_INVALID_ARG: a required pointer NULL; n, t, log_ext, n_public (g, exponents) not a shape of
 *     kzg_circuit_verify_proof (kzg_circuit_custom_verify_proof); proof_len not kzg_circuit_proof_size's; count >
 *     KZG_VERIFY_MAX_PROOFS; n < 2 (w = 1: the two point sets coincide); pi_stride < n_public with count > 1; a shift or a public
 *     input not below r; a key commitment off the curve; a G2 input off the twist; then, from the device, a key commitment
 *     outside G1.
 *   KZG_ERR_NO_SRS: the SRS is empty.  KZG_ERR_HIP: a device call failed, the OS random source did, or the host ran out of memory
 *     or threads for a large batch.
 * The call holds one slot; thread safety and multi-device contexts as kzg_verify_openings_batch (a replicated SRS forwards to
 * one device, a range-split one returns KZG_ERR_INVALID_ARG); the workspaces grow on demand and stay with the context.
 * Not offered: lookup proofs and next-row proofs (their stacks and sets differ), proofs of different keys in one call, locating
 * the invalid proof, hashing on the device.
 * A call costs 12 to 13 ms whatever count is up to a thousand proofs (two dependent ladder launches, the sums, the pairing), so
 * for few proofs kzg_circuit_verify_proof on the host's threads stays the faster route.  Measured (t = 3,
 * e = 4, n = 256, 16 public inputs, the process held to 16 CPUs, medians of five): 13.0 ms against 8.7 for a loop of
 * kzg_circuit_verify_proof over 16 threads at 16 proofs, 12.6 against 16.9 at 32 (the ranges do not overlap), 12.7 against 93 at
 * 256, 13.6 against 355 at 1024, 15.2 against 1347 at 4096.  The crossover lies between 16 and 32 proofs; below it keep using the
 * host verifier. */
#define KZG_VERIFY_MAX_PROOFS (1u << 16)
int kzg_circuit_verify_proofs_batch(kzg_ctx* ctx, const uint64_t* key_p1s, size_t n, size_t t, unsigned log_ext, size_t g,
                                    const uint8_t* exponents, const uint64_t* shifts, const uint64_t* public_inputs, size_t n_public,
                                    size_t pi_stride /* values between proofs */, const uint8_t* proofs, size_t proof_len, size_t count,
                                    const void* setup_g2, size_t g2_stride_bytes, int* valid, size_t* bad_index /* may be NULL */);
/* test hook: the same with the caller's weights (count x blst_fr, any field elements below r; checked after the G2 inputs) instead
 * of random ones; out_p1s receives P0, P1, P2, normalised like kzg_open's output (infinity three times when a proof does not
 * decode), and *valid comes from the same pairing */
int kzg_circuit_verify_proofs_lincomb(kzg_ctx* ctx, const uint64_t* key_p1s, size_t n, size_t t, unsigned log_ext, size_t g,
                                      const uint8_t* exponents, const uint64_t* shifts, const uint64_t* public_inputs, size_t n_public,
                                      size_t pi_stride, const uint8_t* proofs, size_t proof_len, size_t count, const void* setup_g2,
                                      size_t g2_stride_bytes, const uint64_t* weights /* count x blst_fr */, uint64_t out_p1s[54],
                                      int* valid, size_t* bad_index);
/* test hook: ... and with the caller's challenges (count x 5 x blst_fr in the order beta, gamma, alpha, zeta, v, below r; checked
 * after the weights) in the place of the hashed ones, so that a test can put zeta on the domain (zeta = 1, zeta = w^i), which no
 * hashed transcript reaches: the device's scalar kernels then take the paths L_0(1) = 1 and PI(w^i) = PI_i */
int kzg_circuit_verify_proofs_lincomb_challenges(kzg_ctx* ctx, const uint64_t* key_p1s, size_t n, size_t t, unsigned log_ext, size_t g,
                                                 const uint8_t* exponents, const uint64_t* shifts, const uint64_t* public_inputs,
                                                 size_t n_public, size_t pi_stride, const uint8_t* proofs, size_t proof_len, size_t count,
                                                 const void* setup_g2, size_t g2_stride_bytes, const uint64_t* weights /* count x blst_fr */,
                                                 const uint64_t* challenges /* count x 5 x blst_fr */, uint64_t out_p1s[54], int* valid,
                                                 size_t* bad_index);

/* ---- zero-knowledge circuit proofs: the wires, z and T's chunks blinded -------------------------------
 * Notation as above: t wires, e = 2^log_ext, N = e n, Z_H = X^n - 1.  A blinded column agrees with the plain one on H, so z, the
 * gate and the permutation are computed from the same values as without blinding, and kzg_circuit_verify accepts a blinded proof
 * as it is: it sees only commitments, evaluations and one proof.
 *     wires     f~_j = f_j + (b_j0 + b_j1 X) Z_H                                  n + 2 coefficients
 *     product   z~   = z + (c_0 + c_1 X + c_2 X^2) Z_H                            n + 3 coefficients
 *     quotient  T~   = Num(f~, z~) / Z_H, of degree t n + t + 2; L_T = (e - 1) n + t + 3 coefficients are returned, those above
 *               degree t n + t + 2 are zero
 *     chunks    T~_c = T_c + d_c X^n - d_(c-1) for c < e - 1, d_(-1) = d_(e-2) = 0; T_c = coefficients [c n, (c + 1) n) of T~, but
 *               the last chunk T_(e-2) is everything from (e - 2) n to L_T: n + t + 3 coefficients.  sum_c X^(c n) T~_c = T~: the
 *               chunk blinders change the chunks' commitments and r~, not T~.
 * BLINDER ARRAY, the same for every call of one proof: 2 t + 3 + (e - 2) canonical blst_fr in the order (b_00, b_01), ..,
 * (b_(t-1)0, b_(t-1)1), c_0, c_1, c_2, d_0 .. d_(e-3).  A value not below r -> KZG_ERR_INVALID_ARG.  The caller owns the
 * randomness; kzg_circuit_blinders fills such an array from the OS CSPRNG (getrandom, uniform below r by rejection; host only;
 * KZG_ERR_INVALID_ARG for t outside [KZG_CIRCUIT_MIN_COLUMNS, KZG_PQ_MAX_COLUMNS], t + 1 > e or log_ext > KZG_PQ_MAX_LOG_EXT).
 * SHAPE RULE: the blinded circuit calls need N >= t n + t + 4 -- T~ fits and the divisibility test still sees at least one
 * coefficient that must vanish -- else KZG_ERR_INVALID_ARG: (n, t, log_ext) = (4, 3, 2) and (8, 7, 3) are refused, (8, 3, 2) is
 * the smallest legal shape with e = t + 1.  kzg_circuit_blinded_sizes (host only) applies the rule and returns the array's length
 * and L_T (either pointer may be NULL).
 * SRS: a commitment needs as many points as its vector has coefficients -- n + nb for a blinded column, n + t + 3 for the chunks of
 * T~ (every chunk is committed padded to the last one's length) -- and the opening n + t + 2; else KZG_ERR_DEGREE_TOO_HIGH.
 *
 * kzg_blind_evaluations: k columns of n values over H (column c at evals + 4 c stride u64, n a power of two) and nb <= 3 blinders
 * per column (column c at blinders + 4 c nb u64) -> the n + nb coefficients of f + b Z_H per column, column c at out_coeffs + 4 c
 * out_stride u64 (out_stride >= n + nb).  The inverse transform, then a patch of 2 nb coefficients.  Needs no SRS; host pointers,
 * synchronous, devices[0] of a multi-device context.
 * kzg_commit_evaluations_blinded: the same followed by the batched MSM; out_p1s: k x 18 u64, each bit for bit kzg_commit of the
 * blinded coefficients.  Serves the wires (nb = 2) and z (nb = 3).  Multi-device rules of kzg_commit_lagrange.
 *
 * kzg_circuit_quotient_blinded: the arguments of kzg_circuit_quotient without gate_coset (the last round cannot linearise a term
 * of the caller's, so a blinded proof with one could not be finished), plus the blinder array.  The wires and z go values ->
 * coefficients -> patch -> the coset from n + 3 coefficients; the constraints are those of the plain call.  out_coeffs: NULL or L_T
 * coefficients; out_p1s: NULL or the e - 1 commitments [T~_c(s)]G, each bit for bit kzg_commit of the blinded chunk.  A non-zero
 * coefficient of the interpolant at [t n + t + 3, N) -> KZG_ERR_REMAINDER.  The _device form takes kzg_dev_alloc buffers of a
 * single-device context (d_out_coeffs: L_T coefficients, overlapping no input); the blinders and out_p1s stay host pointers.
 *
 * kzg_circuit_open_blinded: the arguments of kzg_circuit_open with t_coeffs = the L_T coefficients above, plus the blinder array.
 * out_evals are the evaluations of the BLINDED polynomials: abar_j = f~_j(zeta), sbar_j = sigma_j(zeta), zw = z~(zeta w).  r~ is
 * r's formula with z~, the T~_c and these evaluations: n + t + 3 coefficients; r~(zeta) != 0 -> KZG_ERR_REMAINDER with the proof
 * unwritten.  The proof is bit for bit kzg_open_sets over [ r~ | f~_0 .. f~_(t-1) | sigma_0 .. sigma_(t-2) | z~ ], each zero-padded
 * to n + t + 3 coefficients, set_of = [0, .., 0, 1], sets {zeta}, {zeta w}, gamma := v.  Statuses (after the NULL pointers, the
 * circuit, the stride and the challenges: the shape rule, then the blinders), locks and multi-device rules are those of
 * kzg_circuit_open.  The _device form: as kzg_circuit_open_device, d_t_coeffs what kzg_circuit_quotient_blinded_device wrote. */
int kzg_circuit_blinded_sizes(size_t n, size_t t, unsigned log_ext, size_t* num_blinders, size_t* quotient_len);
int kzg_circuit_blinders(size_t t, unsigned log_ext, uint64_t* out);
int kzg_blind_evaluations(kzg_ctx* ctx, const uint64_t* evals, size_t n, size_t k, size_t stride, const uint64_t* blinders, size_t nb,
                          uint64_t* out_coeffs, size_t out_stride);
int kzg_commit_evaluations_blinded(kzg_ctx* ctx, const uint64_t* evals, size_t n, size_t k, size_t stride, const uint64_t* blinders,
                                   size_t nb, uint64_t* out_p1s);
int kzg_circuit_quotient_blinded(kzg_ctx* ctx, const kzg_circuit* circuit, const uint64_t* wires, size_t stride, const uint64_t* z,
                                 const uint64_t* public_inputs, const uint64_t alpha[4], const uint64_t beta[4], const uint64_t gamma[4],
                                 const uint64_t* blinders, uint64_t* out_coeffs, uint64_t* out_p1s);
int kzg_circuit_quotient_blinded_device(kzg_ctx* ctx, const kzg_circuit* circuit, const void* d_wires, size_t stride, const void* d_z,
                                        const void* d_public_inputs, const uint64_t alpha[4], const uint64_t beta[4],
                                        const uint64_t gamma[4], const uint64_t* blinders, void* d_out_coeffs, uint64_t* out_p1s);
int kzg_circuit_open_blinded(kzg_ctx* ctx, const kzg_circuit* circuit, const uint64_t* wires, size_t stride, const uint64_t* z,
                             const uint64_t* public_inputs, const uint64_t* t_coeffs, const uint64_t alpha[4], const uint64_t beta[4],
                             const uint64_t gamma[4], const uint64_t zeta[4], const uint64_t v[4], const uint64_t* blinders,
                             uint64_t* out_evals, uint64_t out_p1[18]);
int kzg_circuit_open_blinded_device(kzg_ctx* ctx, const kzg_circuit* circuit, const void* d_wires, size_t stride, const void* d_z,
                                    const void* d_public_inputs, const void* d_t_coeffs, const uint64_t alpha[4],
                                    const uint64_t beta[4], const uint64_t gamma[4], const uint64_t zeta[4], const uint64_t v[4],
                                    const uint64_t* blinders, uint64_t* out_evals, uint64_t out_p1[18]);

/* ---- every cell of a domain and its multiproof ----------------------------------------------
 * Domain of N = 2^log_domain points (w_N as kzg_domain_root), cells of l = 2^log_cell points: cell j (j < N / l) is the
 * coset {w_N^(j + (N/l) i) : i < l}, whose vanishing polynomial is X^l - w_N^(j l).  Its proof is exactly what
 * kzg_open_points returns for its l points and values (for l = 1: kzg_open's at w_N^j), all N / l of them from one
 * call: the quotients are stride-l synthetic divisions on the device and the proofs batched MSMs over the SRS.
 * n' = n without trailing zeros.  Errors: log_domain > KZG_NTT_MAX_LOG, log_cell > KZG_MAX_CELL_LOG, log_cell >
 *   log_domain, n > N, a required pointer NULL (evaluations: n not a power of two) -> KZG_ERR_INVALID_ARG; then no SRS
 *   -> KZG_ERR_NO_SRS; n' - l > kzg_srs_len -> KZG_ERR_DEGREE_TOO_HIGH.  n' <= l gives infinity proofs, n = 0 zero cells
 *   too; there is no constant-polynomial error.  Thread-safe on one context like the other host-pointer calls.
 * Sampling specs list the N values in bit-reversed order (brp_b: b-bit bit reversal, K = log_domain, t = log_cell):
 *   their cell c (positions c l .. c l + l - 1) is this API's cell brp_(K-t)(c), its values are out_cells of that cell
 *   in brp_t(i) order, and its proof is identical.  Nothing is bit-reversed at the boundary (as for kzg_ntt).
 * Multi-device contexts: a replicated SRS forwards the call to one device; a range-split SRS returns
 *   KZG_ERR_INVALID_ARG (kzg_last_error says why).  kzg_quotient_cells runs on devices[0]. */
#define KZG_MAX_CELL_LOG 6 /* l <= 64 = KZG_MAX_OPEN_POINTS */
/* P by coefficients (n x blst_fr, Montgomery), N = 2^log_domain, l = 2^log_cell.
 * out_cells (may be NULL): N x 4 u64, cell-major: out_cells[4 (j l + i) ..] = P(w_N^(j + (N/l) i)).
 * out_proofs: (N/l) x 18 u64 (blst_p1, normalised like kzg_open's output, all-zero = infinity). */
int kzg_cells_and_proofs(kzg_ctx* ctx, const uint64_t* coeffs_fr_mont, size_t n, unsigned log_domain, unsigned log_cell,
                         uint64_t* out_cells, uint64_t* out_proofs);
/* P by its values over the n-domain (n a power of two <= N, natural order, as kzg_commit_evaluations takes them),
 * extended to N on the device */
int kzg_cells_and_proofs_evaluations(kzg_ctx* ctx, const uint64_t* evals_fr_mont, size_t n, unsigned log_domain,
                                     unsigned log_cell, uint64_t* out_cells, uint64_t* out_proofs);
/* test hook, like kzg_quotient_points: quotients of cells [first_cell, first_cell + count), cell c at
 * out_q + 4 (c - first_cell) (n - l); *out_qn = max(n' - l, 0) (entries past it are zero); no SRS needed */
int kzg_quotient_cells(kzg_ctx* ctx, const uint64_t* coeffs_fr_mont, size_t n, unsigned log_domain, unsigned log_cell,
                       size_t first_cell, size_t count, uint64_t* out_q, size_t* out_qn);

/* ---- every cell proof of many polynomials by FK20 -------------------------------------------
 * kzg_cells_and_proofs for `batch` polynomials of n coefficients (polynomial b at coeffs + 4*b*stride_coeffs), by FK20:
 * the N/l proofs are a G1 DFT of size N/l of l Toeplitz products, O(n log n) group operations instead of N (n - l) / l
 * MSM terms.  out_cells (may be NULL): batch x N x 4 u64; out_proofs: batch x (N/l) x 18 u64.
 * Every output equals what kzg_cells_and_proofs returns for that polynomial, bit for bit, error codes included (n' per
 * polynomial; a degree error anywhere fails the whole call and kzg_last_error names the polynomial).  batch = 0 does
 * nothing; stride_coeffs < n with batch > 1 -> KZG_ERR_INVALID_ARG.  One exception to the cells call's acceptance: a
 * shape whose circulant length L (the power of two >= 2 ceil(n_max / l), n_max the largest n' of the batch) exceeds
 * 2^22 = the largest root of the twiddle tables returns KZG_ERR_INVALID_ARG; that needs l = 1 and n' > 2^21.
 * The SRS-side transforms for (L, l) are built on first use (or by kzg_fk20_prepare) and kept per context, one shape at
 * a time, until the SRS is replaced: l L x 256 B of transforms, plus their comb tables (l L x 64 KiB: 512 MiB at n = 4096,
 * l = 64) when those fit KZG_FK20_TABLE_MB, by default a quarter of the free device memory up to 16 GiB.  Larger shapes
 * build the comb tables per call, 8192 bases at a time, and free them again; no size is refused for memory.  A kept
 * transform of the same l and up to twice the needed L serves shorter polynomials without a rebuild.  Thread-safe: FK20
 * calls on one context run one after the other, other calls go on while one waits for the device. */
int kzg_cells_and_proofs_fk20(kzg_ctx* ctx, const uint64_t* coeffs_fr_mont, size_t n, size_t batch, size_t stride_coeffs,
                              unsigned log_domain, unsigned log_cell, uint64_t* out_cells, uint64_t* out_proofs);
/* optional: build the SRS-side cache for polynomials of n coefficients and cells of 2^log_cell points now */
int kzg_fk20_prepare(kzg_ctx* ctx, size_t n, unsigned log_cell);

/* ---- recovery of every cell and proof from part of the cells --------------------------------
 * Cells as in kzg_cells_and_proofs: N = 2^log_domain, l = 2^log_cell, M = N / l cells, value i of cell j is
 * P(w_N^(j + M i)).  Given k distinct received cells (cell_ids[t] < M, any order) of `batch` polynomials of n coefficients,
 * with k l >= n, the call rebuilds each polynomial on the device (an erasure decode over the coset 7 <w_N>, DESIGN.md
 * section 4.9) and returns what is requested:
 *   out_coeffs (may be NULL): batch x n x 4 u64, canonical; entries past n' are zero.
 *   out_cells  (may be NULL): batch x N x 4 u64, cell-major;  out_proofs (may be NULL): batch x M x 18 u64 (blst_p1).
 *   Both are bit for bit what kzg_cells_and_proofs_fk20 (= kzg_cells_and_proofs) returns for the recovered coefficients,
 *   so the received cells come back unchanged.  All three NULL only validates.
 * Input: value i of received cell t (cell cell_ids[t]) of polynomial b at cells + 4 ((b k + t) l + i).  One set of cell
 *   ids serves the whole batch (the blobs of one block arrive with the same indices); callers with different sets make one
 *   call per set.  Sampling specs that list the N values in bit-reversed order: their cell c is this API's cell
 *   brp_(K-t)(c) and its values are in brp_t(i) order (as for kzg_cells_and_proofs).
 * Errors, in this order:
 *   KZG_ERR_INVALID_ARG: log_domain > KZG_NTT_MAX_LOG, log_cell > KZG_MAX_CELL_LOG, log_cell > log_domain,
 *     log_domain - log_cell > KZG_RECOVER_MAX_LOG_CELLS; n = 0 or n > N; k l < n; a cell id >= M or a duplicate; a
 *     required pointer NULL; an input value >= r (checked on the host: recovery input comes from the network;
 *     kzg_last_error names the polynomial and the cell).
 *   KZG_ERR_NO_SRS: out_proofs requested without an SRS (coefficients and cells need none).
 *   KZG_ERR_REMAINDER: the received values of some polynomial are not those of a polynomial of fewer than n coefficients
 *     (its decoded coefficients at [n, N) are not all zero); kzg_last_error names the first one, the whole call fails.
 *   KZG_ERR_DEGREE_TOO_HIGH: as kzg_cells_and_proofs_fk20 returns it when proofs are requested (n' - l > kzg_srs_len).
 * batch = 0 does nothing.  Thread safety and multi-device contexts as kzg_cells_and_proofs_fk20 (a replicated SRS forwards
 * to one device, a range-split one returns KZG_ERR_INVALID_ARG).  The cost of the vanishing evaluations grows as M (N - k l)
 * / l, hence the cap on M. */
#define KZG_RECOVER_MAX_LOG_CELLS 13 /* M = N / l <= 8192 */
int kzg_recover_cells_and_proofs(kzg_ctx* ctx, size_t n, unsigned log_domain, unsigned log_cell, const uint32_t* cell_ids,
                                 size_t k, const uint64_t* cells, size_t batch, uint64_t* out_coeffs, uint64_t* out_cells,
                                 uint64_t* out_proofs);
/* ---- batch verification of cell proofs: one pairing check for many cells ------------------------------------------
 * Cells as in kzg_cells_and_proofs: N = 2^log_domain, l = 2^log_cell, M = N / l; value i of cell j is P(w_N^(j + M i)), cell j
 * is the coset h_j <w_l> with h_j = w_N^j and X^l = a_j = w_M^j on it.  Record t (t < k) claims that commitment
 * commitment_idx[t] opens to the l values at cells + 4 (t l + i) (blst_fr, Montgomery) on cell cell_ids[t], with the proof at
 * proofs_p1 + 18 t:  e(pi_t, [s^l - a_j]G2) == e(C_b - [I_t(s)]G1, G2), I_t the interpolant of the values on the coset.
 * The call checks all records at once: with weights rho_t = a_t + b_t lambda (a_t, b_t uniform
 * 64-bit from the OS CSPRNG, getrandom(2), fresh on every call; lambda = z^2 - 1) it forms on the device
 *     LHS = sum_t rho_t pi_t,    RHS = sum_b U_b C_b - [A(s)]G1 + sum_j [a_j] T_j
 * (U_b = sum of the weights of b's records, T_j = sum_{t: j_t = j} rho_t pi_t, A = sum_t rho_t I_t) and pairs once on the host:
 * e(LHS, [s^l]G2) == e(RHS, G2).  *valid = 1 when every record is valid; a batch with an invalid record is accepted with
 * probability at most 2^-128.  The weights are not the Fiat-Shamir weights of the sampling specs (no hashing of the
 * inputs): the boolean answer is the same, the randomness is the caller's process's.
 * Inputs: points are blst_p1 (all-zero: infinity); [s^t]G1 for t < l comes from the context's SRS; setup_g2 is read at indices
 * 0 ([1]G2) and l ([s^l]G2), g2_stride_bytes apart, as kzg_verify_points reads it.  Repeated records and repeated cell ids
 * are allowed; k = 0 gives *valid = 1.  Sampling specs that list the N values in bit-reversed order: their cell c is this
 * API's cell brp_(log_domain - log_cell)(c) and its values are in brp_(log_cell)(i) order (as for kzg_cells_and_proofs).
 * Errors (kzg_last_error names the record or the commitment):
 *   KZG_ERR_INVALID_ARG: log_domain > KZG_NTT_MAX_LOG, log_cell > KZG_MAX_CELL_LOG, log_cell > log_domain; k or
 *     num_commitments > KZG_VERIFY_MAX_CELLS; a required pointer NULL; commitment_idx[t] >= num_commitments; cell_ids[t] >= M;
 *     a value >= r (checked on the host); a G1 coordinate not below p; a G2 input off the twist; then, from the device, a
 *     proof or commitment off the curve or outside G1 (the order-r subgroup; infinity passes).
 *   KZG_ERR_NO_SRS: the SRS holds fewer than l points.
 *   KZG_ERR_HIP: a device call failed, or the OS random source did.
 * Thread safety as kzg_cells_and_proofs_fk20 (the call holds one slot and waits without the context lock); a replicated
 * multi-device context forwards to one device, a range-split one returns KZG_ERR_INVALID_ARG. */
#define KZG_VERIFY_MAX_CELLS (1u << 20)
int kzg_verify_cells_batch(kzg_ctx* ctx, const uint64_t* commitments_p1, size_t num_commitments, const uint32_t* commitment_idx,
                           const uint32_t* cell_ids, const uint64_t* cells, const uint64_t* proofs_p1, size_t k, unsigned log_domain,
                           unsigned log_cell, const void* setup_g2, size_t g2_stride_bytes, int* valid);
/* test hook: the same with the caller's weights (k x blst_fr, any field elements below r) instead of random ones; returns the
 * two G1 sides, normalised like kzg_open's output (Z = Montgomery one, or all zero for infinity), and *valid from the same
 * pairing */
int kzg_verify_cells_lincomb(kzg_ctx* ctx, const uint64_t* commitments_p1, size_t num_commitments, const uint32_t* commitment_idx,
                             const uint32_t* cell_ids, const uint64_t* cells, const uint64_t* proofs_p1, size_t k,
                             unsigned log_domain, unsigned log_cell, const void* setup_g2, size_t g2_stride_bytes,
                             const uint64_t* weights, uint64_t out_lhs_p1[18], uint64_t out_rhs_p1[18], int* valid);
/* ---- openings at arbitrary points: evaluation of polynomials in evaluation form, one pairing for many openings ---------
 * (DESIGN.md section 4.11).
 * kzg_evaluate_evaluations_batch: P_b by its values over the n-domain (n = 2^k <= 2^KZG_NTT_MAX_LOG, natural order, as
 * kzg_commit_evaluations takes them), polynomial b at evals + 4 b stride; out_ys[4 b ..] = P_b(z_b), canonical blst_fr.  The
 * barycentric formula P(z) = (z^n - 1) / n sum_i f_i w^i / (z - w^i) on the device, no interpolation; a point inside the domain
 * returns the value held there.  Needs no SRS.  Batches larger than a slot's staging buffers run in chunks.
 * Errors: KZG_ERR_INVALID_ARG: n not a power of two or too large; a required pointer NULL; stride < n with batch > 1; a point
 * or a value >= r (checked on the host; kzg_last_error names the polynomial).  batch = 0 does nothing; n = 1 returns the
 * constant.  Thread safety as kzg_ntt (one slot per call); multi-device contexts run it on their first device. */
int kzg_evaluate_evaluations_batch(kzg_ctx* ctx, const uint64_t* evals_fr_mont, size_t n, size_t batch, size_t stride,
                                   const uint64_t* zs, uint64_t* out_ys);
/* kzg_verify_openings_batch: record t (t < k) claims that commitment commitment_idx[t] opens to ys + 4 t at the point zs + 4 t
 * (blst_fr, Montgomery, any field elements: challenges, not domain indices) with the proof at proofs_p1 + 18 t -- the claim
 * kzg_verify_proof checks with two pairings per record.  With the weights of kzg_verify_cells_batch (rho_t = a_t + b_t lambda,
 * a_t, b_t uniform 64-bit from getrandom(2), fresh on every call) the device forms
 *     LHS = sum_t rho_t pi_t,    RHS = sum_b U_b C_b - [sum_t rho_t y_t]G1 + sum_z [z] T_z,    T_z = sum_{t: z_t = z} rho_t pi_t
 * and the host pairs once: e(LHS, [s]G2) == e(RHS, G2).  *valid = 1 when every record is valid; a batch with an invalid
 * record is accepted with probability at most 2^-128.  The records are grouped by distinct point: one point shared by many
 * polynomials costs one full scalar multiplication, every record a 64-step one.
 * Inputs: points are blst_p1 (all-zero: infinity); [1]G1 is the context's SRS[0]; setup_g2 is read at indices 0 ([1]G2) and 1
 * ([s]G2), g2_stride_bytes apart, as kzg_verify_points reads it.  Repeated records and repeated points are allowed; k = 0
 * gives *valid = 1.
 * Errors (kzg_last_error names the record or the commitment):
 *   KZG_ERR_INVALID_ARG: k or num_commitments > KZG_VERIFY_MAX_OPENINGS; a required pointer NULL; commitment_idx[t] >=
 *     num_commitments; a point or a value >= r (checked on the host); a G1 coordinate not below p; a G2 input off the twist;
 *     then, from the device, a proof or commitment off the curve or outside G1 (the order-r subgroup; infinity passes).
 *   KZG_ERR_NO_SRS: the SRS is empty.
 *   KZG_ERR_HIP: a device call failed, or the OS random source did.
 * Thread safety and multi-device contexts as kzg_verify_cells_batch (a replicated SRS forwards to one device, a range-split one
 * returns KZG_ERR_INVALID_ARG).  A call costs about 10 ms whatever k is up to some thousand records, so for few records
 * kzg_verify_proof_batch on the host (min(hardware threads, n) threads) stays the faster route.  Measured crossover (DESIGN.md
 * section 5.0f): between 32 and 48 records with the process held to 16 CPUs, between 256 and 384 records with all 256 CPUs
 * of the same box open to it.  Below it keep using the host batch. */
#define KZG_VERIFY_MAX_OPENINGS (1u << 20)
int kzg_verify_openings_batch(kzg_ctx* ctx, const uint64_t* commitments_p1, size_t num_commitments, const uint32_t* commitment_idx,
                              const uint64_t* zs, const uint64_t* ys, const uint64_t* proofs_p1, size_t k, const void* setup_g2,
                              size_t g2_stride_bytes, int* valid);
/* test hook: the same with the caller's weights (k x blst_fr, any field elements below r) instead of random ones; returns the
 * two G1 sides, normalised like kzg_open's output, and *valid from the same pairing */
int kzg_verify_openings_lincomb(kzg_ctx* ctx, const uint64_t* commitments_p1, size_t num_commitments, const uint32_t* commitment_idx,
                                const uint64_t* zs, const uint64_t* ys, const uint64_t* proofs_p1, size_t k, const void* setup_g2,
                                size_t g2_stride_bytes, const uint64_t* weights, uint64_t out_lhs_p1[18], uint64_t out_rhs_p1[18],
                                int* valid);
/* The two together, for a verifier that holds the polynomials in evaluation form (blobs): polynomial b (laid out as for
 * kzg_evaluate_evaluations_batch) is claimed to have commitment commitments_p1 + 18 b and the opening proof proofs_p1 + 18 b at
 * the caller's challenge zs + 4 b.  The values y_b = P_b(z_b) are computed on the device and go into the check without
 * leaving it; out_ys (batch x blst_fr, may be NULL) receives them.  The challenges are the caller's (no hashing here).
 * Errors: those of the two calls above (batch in the place of k and of num_commitments). */
int kzg_verify_evaluations_batch(kzg_ctx* ctx, const uint64_t* evals_fr_mont, size_t n, size_t batch, size_t stride,
                                 const uint64_t* commitments_p1, const uint64_t* zs, const uint64_t* proofs_p1,
                                 const void* setup_g2, size_t g2_stride_bytes, uint64_t* out_ys, int* valid);
/* test hook: DFT (inverse != 0: inverse DFT incl. 1/m) of m = 2^k <= 2^22 host blst_p1 points over w_m, normalised
 * output (out_p1[j] = sum_i [w_m^(i j)] in_p1[i]); needs no SRS.  The points must lie in G1 (the order-r subgroup): the
 * twiddle products use the endomorphism (x, y) -> (beta x, y) = [z^2 - 1](x, y), which holds there only; nothing checks it */
int kzg_g1_dft(kzg_ctx* ctx, const uint64_t* in_p1, size_t m, int inverse, uint64_t* out_p1);

/* ---- the batch verifiers on inputs as they travel ------------------------------------------------
 * A sampling node receives commitments and proofs as 48-byte compressed G1 points (ZCash encoding, as kzg_g1_compress writes
 * them), field elements as 32-byte big-endian strings, and cells and blobs in the bit-reversed order of the sampling specs.
 * The calls below take exactly that: the bytes are uploaded as received and decoded on the device (one lane per point: the
 * 381-bit square root; one lane per value) straight into the buffers the verifiers read, instead of one kzg_g1_uncompress
 * per point and a conversion per value on the host.  For inputs that decode, each returns what its sibling without _bytes
 * returns on the decoded inputs: the same *valid, and the same two sides bit for bit from the _lincomb hooks.
 * order: KZG_ORDER_NATURAL -- cells, their values and a blob's values as this API defines them; KZG_ORDER_BIT_REVERSED -- the
 * sampling specs' view of the same data: cell_ids[t] = c names this API's cell brp(c) (bit reversal over log_domain -
 * log_cell bits), its values arrive with value i at this API's position brp(i) (log_cell bits), and value i of a blob of n
 * values is this API's value brp(i) (log2 n bits).
 * Decoding: a point is accepted as blst_p1_uncompress accepts it (compressed flag set; infinity is 0xc0 followed by zeros;
 * otherwise x < p and x^3 + 4 a square; the sign bit chooses y), membership in G1 is then checked as in the siblings; a scalar
 * must be below r.  The points zs of the openings are decoded on the host (it groups the records by point), all else on the
 * device.
 * Errors: those of the siblings, in their order, up to where they read a G1 coordinate or a value; an order that is neither
 * constant is KZG_ERR_INVALID_ARG; then KZG_ERR_INVALID_ARG with kzg_last_error naming the input: "the proof of record t" /
 * "commitment b" "is not a valid compressed point" (flag bits, malformed infinity, x >= p, x not on the curve) or "is not in
 * G1"; "record t: value i" (i as sent), "record t: the point z", "record t: the claimed y", "polynomial b: value i" /
 * "polynomial b: the point z" "is not below r" (these are the _bytes calls' wordings; the siblings, which check decoded
 * scalars on the host, say "record t: the point" / "record t: the value").  When several inputs are bad, one of them is named.  A flipped sign bit is the
 * valid point -P: KZG_OK with *valid = 0.  Infinity passes wherever the siblings let it pass.
 * Thread safety and multi-device contexts as the siblings (one slot per call; a replicated SRS forwards to one device, a
 * range-split one returns KZG_ERR_INVALID_ARG); kzg_verify_blobs_batch_bytes runs large batches in chunks as
 * kzg_evaluate_evaluations_batch does.  What the decode costs against the host route: DESIGN.md section 5.0g. */
#define KZG_ORDER_NATURAL 0u
#define KZG_ORDER_BIT_REVERSED 1u
/* kzg_verify_cells_batch on k records of cells_be + 32 (t l + i) (k x l x 32 bytes), proofs48 + 48 t, commitments48 + 48 b */
int kzg_verify_cells_batch_bytes(kzg_ctx* ctx, const uint8_t* commitments48, size_t num_commitments, const uint32_t* commitment_idx,
                                 const uint32_t* cell_ids, const uint8_t* cells_be, const uint8_t* proofs48, size_t k,
                                 unsigned log_domain, unsigned log_cell, unsigned order, const void* setup_g2, size_t g2_stride_bytes,
                                 int* valid);
/* test hook, as kzg_verify_cells_lincomb: the caller's weights (k x blst_fr), the two sides out */
int kzg_verify_cells_lincomb_bytes(kzg_ctx* ctx, const uint8_t* commitments48, size_t num_commitments, const uint32_t* commitment_idx,
                                   const uint32_t* cell_ids, const uint8_t* cells_be, const uint8_t* proofs48, size_t k,
                                   unsigned log_domain, unsigned log_cell, unsigned order, const void* setup_g2,
                                   size_t g2_stride_bytes, const uint64_t* weights, uint64_t out_lhs_p1[18], uint64_t out_rhs_p1[18],
                                   int* valid);
/* kzg_verify_openings_batch on zs_be + 32 t, ys_be + 32 t, proofs48 + 48 t, commitments48 + 48 b */
int kzg_verify_openings_batch_bytes(kzg_ctx* ctx, const uint8_t* commitments48, size_t num_commitments, const uint32_t* commitment_idx,
                                    const uint8_t* zs_be, const uint8_t* ys_be, const uint8_t* proofs48, size_t k,
                                    const void* setup_g2, size_t g2_stride_bytes, int* valid);
int kzg_verify_openings_lincomb_bytes(kzg_ctx* ctx, const uint8_t* commitments48, size_t num_commitments,
                                      const uint32_t* commitment_idx, const uint8_t* zs_be, const uint8_t* ys_be,
                                      const uint8_t* proofs48, size_t k, const void* setup_g2, size_t g2_stride_bytes,
                                      const uint64_t* weights, uint64_t out_lhs_p1[18], uint64_t out_rhs_p1[18], int* valid);
/* kzg_verify_evaluations_batch for blobs as they travel: blob b is n x 32 big-endian bytes at blobs_be + 32 b stride (stride in
 * values, >= n), its commitment at commitments48 + 48 b, its proof at proofs48 + 48 b, the challenge at zs_be + 32 b.
 * out_ys_be (batch x 32 bytes, may be NULL) receives the big-endian image of what kzg_verify_evaluations_batch writes to
 * out_ys. */
int kzg_verify_blobs_batch_bytes(kzg_ctx* ctx, const uint8_t* blobs_be, size_t n, size_t batch, size_t stride, unsigned order,
                                 const uint8_t* commitments48, const uint8_t* zs_be, const uint8_t* proofs48, const void* setup_g2,
                                 size_t g2_stride_bytes, uint8_t* out_ys_be, int* valid);
/* building blocks and test hooks: n compressed points -> n blst_p1 (Z = Montgomery one, all zero = infinity) decoded on the
 * device, each equal to what kzg_g1_uncompress returns; check_subgroup != 0 also requires each to lie in G1.  n x 32
 * big-endian bytes -> n blst_fr.  On a bad input: KZG_ERR_INVALID_ARG and *bad_index = the least bad index ((size_t)-1
 * otherwise; bad_index may be NULL).  n = 0 does nothing.  They need no SRS; thread safety as kzg_g1_dft; multi-device
 * contexts run them on their first device. */
int kzg_g1_uncompress_batch(kzg_ctx* ctx, const uint8_t* in48, size_t n, int check_subgroup, uint64_t* out_p1, size_t* bad_index);
int kzg_fr_from_bytes_batch(kzg_ctx* ctx, const uint8_t* in32_be, size_t n, uint64_t* out_fr_mont, size_t* bad_index);

/* ---- the producing side on blobs as they travel ----------------------------------------------------
 * The mirror of the section above: a block builder or a node that reconstructs data holds blobs as bytes, in evaluation form,
 * and wants 48-byte commitments, 48-byte proofs and cell bytes.  The calls below take the blob bytes as they are and return
 * exactly those: the values are decoded on the device, interpolated there (one batched inverse transform), and the coefficients
 * stay resident for the commitments (the batched MSM), the cells (one batched transform and gather) and the FK20 proofs; points
 * and values are encoded on the device (one lane each) and leave in one download per chunk of polynomials.  The
 * coefficients never visit the host, and it converts no value and no proof; the commitments alone come off the MSM's host tail as
 * blst_p1 and are compressed there, one host compression per blob.
 * Blob b is n x 32 big-endian bytes at blobs_be + 32 b stride (stride in values, >= n when batch > 1): the values of P_b over
 * the n-domain as kzg_commit_evaluations takes them, n a power of two <= 2^KZG_NTT_MAX_LOG and <= N = 2^log_domain.  order as
 * in kzg_verify_blobs_batch_bytes: with KZG_ORDER_BIT_REVERSED, value i as sent is this API's value brp(i) over log2 n bits.
 * Outputs: out_commitments48 + 48 b; out_cells_be, batch x N x 32 bytes; out_proofs48, batch x (N / l) x 48 bytes.  With
 * KZG_ORDER_NATURAL, cells and proofs are in this API's cell-major order and numbering.  With KZG_ORDER_BIT_REVERSED they are in
 * the specs' order: slot c holds this API's cell brp(c) over log_domain - log_cell bits with its values in brp order over
 * log_cell bits, and the proof in slot c is that cell's -- the mappings stated above for kzg_verify_cells_batch_bytes.
 * Meaning, for inputs that decode: the commitment is kzg_g1_compress(kzg_commit_evaluations(decoded blob)); cells and proofs
 * are those of kzg_cells_and_proofs_fk20 on the interpolated coefficients, encoded; byte for byte (every quantity is exact
 * arithmetic with one canonical encoding).  kzg_recover_cells_and_proofs_bytes takes and returns what
 * kzg_recover_cells_and_proofs does for the decoded input (cells_be: batch x k x l x 32 bytes); cell_ids and the values inside
 * a cell follow `order`; it has no coefficient output.
 * Errors, in this order: KZG_ERR_INVALID_ARG for the shape, an order that is neither constant, a NULL required pointer, stride <
 * n with batch > 1; KZG_ERR_NO_SRS; KZG_ERR_INVALID_ARG from the device with kzg_last_error naming "polynomial b: value i is not
 * below r" (recovery: "polynomial b, cell c: value i is not below r"; i, and c, as sent); KZG_ERR_REMAINDER for recovery, as its
 * sibling; KZG_ERR_DEGREE_TOO_HIGH when n' > kzg_srs_len and commitments are asked for, or n' - l > kzg_srs_len for proofs (n'
 * = 1 + the degree of the interpolated polynomial; kzg_last_error names the polynomial).  batch = 0 does nothing.  A failed call
 * writes no output the caller may rely on.
 * Thread safety as kzg_cells_and_proofs_fk20 (the calls share its workspaces and queue behind one another); a replicated
 * multi-device context forwards to one device, a range-split one returns KZG_ERR_INVALID_ARG.  Polynomials go through the
 * workspaces in chunks, as in kzg_cells_and_proofs_fk20.
 * Measured (MI355X, n = 4096, log_domain 13, log_cell 6, KZG_ORDER_BIT_REVERSED, all three outputs,
 * medians of three repetitions): 64 blobs per call 50.7-51.1 ms, against 106.3-108.8 ms for the existing entry points chained by
 * hand (kzg_fr_from_bytes_batch, kzg_ntt per blob, kzg_commit_batch, kzg_cells_and_proofs_fk20, kzg_g1_compress per point).
 * There is no crossover down to 1 blob per call, and no gain to speak of there either: 31.5-31.9 ms against 32.6 ms, both being
 * the time FK20 takes for one polynomial. */
int kzg_blobs_to_commitments_bytes(kzg_ctx* ctx, const uint8_t* blobs_be, size_t n, size_t batch, size_t stride, unsigned order,
                                   uint8_t* out_commitments48);
int kzg_blobs_to_cells_and_proofs_bytes(kzg_ctx* ctx, const uint8_t* blobs_be, size_t n, size_t batch, size_t stride,
                                        unsigned log_domain, unsigned log_cell, unsigned order,
                                        uint8_t* out_commitments48 /* may be NULL */, uint8_t* out_cells_be /* may be NULL */,
                                        uint8_t* out_proofs48);
int kzg_recover_cells_and_proofs_bytes(kzg_ctx* ctx, size_t n, unsigned log_domain, unsigned log_cell, unsigned order,
                                       const uint32_t* cell_ids, size_t k, const uint8_t* cells_be, size_t batch,
                                       uint8_t* out_cells_be /* may be NULL */, uint8_t* out_proofs48 /* may be NULL */);
/* building blocks and test hooks, the inverses of kzg_g1_uncompress_batch / kzg_fr_from_bytes_batch: n blst_p1 (any Z; all zero
 * = infinity) -> n x 48 bytes, each what kzg_g1_compress returns for that point (normalised and encoded on the device); n
 * blst_fr -> n x 32 big-endian bytes, a value not below r giving KZG_ERR_INVALID_ARG and *bad_index = the least bad index
 * ((size_t)-1 otherwise; bad_index may be NULL).  n = 0 does nothing.  They need no SRS; thread safety as kzg_g1_dft;
 * multi-device contexts run them on their first device. */
int kzg_g1_compress_batch(kzg_ctx* ctx, const uint64_t* in_p1, size_t n, uint8_t* out48);
int kzg_fr_to_bytes_batch(kzg_ctx* ctx, const uint64_t* in_fr_mont, size_t n, uint8_t* out32_be, size_t* bad_index);

/* ---- blob proofs and their Fiat-Shamir challenges --------------------------------------------------
 * The proof that travels with a blob, and the challenge it is bound to: compute_kzg_proof, compute_blob_kzg_proof and
 * verify_blob_kzg_proof_batch of the blob specs, for batches, on bytes.  Blobs, n, batch, stride and order as in the section
 * above.
 * The challenge of blob b with commitment C_b is
 *     z_b = int_be(SHA256("FSBLOBVERIFY_V1_" | n as 16 bytes big-endian | the n x 32 blob bytes as sent | the 48 bytes of C_b)) mod r.
 * The blob bytes enter the hash as they were sent, whatever `order` says (bytes between n and stride are not part of a blob),
 * and the 48 commitment bytes enter it AS GIVEN: they are neither decoded nor checked here.
 * kzg_sha256 is the hash on its own: a building block and test hook.  It runs on the x86 SHA extensions where CPUID reports
 * them (kzg_sha256_has_shani returns 1) and in portable C++ otherwise.  kzg_sha256_pieces feeds the same bytes through the
 * streaming interface `piece` bytes at a time on the path asked for -- KZG_SHA256_AUTO, KZG_SHA256_PORTABLE or
 * KZG_SHA256_SHANI (KZG_ERR_INVALID_ARG on a CPU without the extensions).  kzg_blob_challenges_bytes writes the challenges, batch x 32 bytes
 * big-endian, each below r.  Both are host-only and need no context: KZG_ERR_INVALID_ARG for a NULL pointer with something
 * to do, n that is no power of two up to 2^KZG_NTT_MAX_LOG, or stride < n with batch > 1; batch = 0 does nothing.  Blobs are
 * hashed on min(batch, 16, hardware threads) threads (the environment variable KZG_HASH_THREADS = 1 .. 15 lowers the 16: for
 * measurements).
 * kzg_blobs_open_at_bytes: y_b = P_b(z_b) and the proof of that opening, for points the caller names (zs_be, batch x 32
 * bytes, each below r).  y is an OUTPUT: there is no claim, hence no KZG_ERR_REMAINDER and no KZG_ERR_CONSTANT_POLY.  A
 * polynomial with n' <= 1 gets the infinity proof (0xc0 and zeros) and y = c_0.  z may lie inside the domain; y is then the
 * blob's own value there.  For every blob the proof is kzg_g1_compress(kzg_open_evaluations(decoded values, z, y)) and y is
 * what kzg_evaluate_evaluations_batch returns, byte for byte.
 * kzg_blobs_to_blob_proofs_bytes: the same at the challenges, derived from commitments48 when given (hashed as given; no
 * commitment is computed) and from the commitments computed here otherwise (those of kzg_blobs_to_commitments_bytes;
 * returned when out_commitments48 is given, which also receives a copy of given ones).  y is not returned.
 * kzg_verify_blob_proofs_batch_bytes: kzg_verify_blobs_batch_bytes with the challenges derived instead of given -- the same
 * answers and the same error wordings as that call with those points.  The batch weights of the one pairing check stay random
 * (the CSPRNG), not the specs' hashed ones: a verdict is the specs' verdict up to the 2^-255 soundness error of either choice.
 * Route: the values are decoded and interpolated on the device as above and the coefficients stay resident; the quotients of
 * all polynomials of a chunk come from ONE launch for n <= 4096 (blobproof_kernels.hip; for larger n the per-polynomial
 * loop of kzg_open_batch runs), the proofs from the batched MSM over them in sub-batches of kzg_max_batch over the stream
 * slots, compressed on the host.  The host hashes the blobs while the device commits.
 * Errors, in this order: KZG_ERR_INVALID_ARG with kzg_last_error for the shape, an order that is neither constant, a NULL
 * required pointer, stride < n with batch > 1, "polynomial b: the point z is not below r"; KZG_ERR_NO_SRS; KZG_ERR_INVALID_ARG
 * from the device naming "polynomial b: value i is not below r" (i as sent); KZG_ERR_DEGREE_TOO_HIGH when n' > kzg_srs_len and
 * commitments are computed, or n' - 1 > kzg_srs_len (kzg_last_error names the polynomial).  batch = 0 does nothing.  A failed
 * call writes no output the caller may rely on.  Thread safety, chunking and multi-device contexts as in the section above.
 * With kzg_set_timing, kzg_get_times of the slot the call leased (the lowest idle one) reports quotient_ms of its last chunk.
 * Measured (MI355X, n = 4096, KZG_ORDER_BIT_REVERSED, kzg_set_max_batch(64), medians of three repetitions
 * with their minimum and maximum): the quotients of 64 polynomials 0.061 ms (0.061-0.062) in the one launch against 2.31 ms
 * (2.31-2.32) in the loop of kzg_open_batch_submit; kzg_blobs_to_blob_proofs_bytes with commitments computed, 64 blobs per call
 * 4.98 ms (4.97-5.02) against 29.1 ms (29.1-30.4) for hashlib, kzg_fr_from_bytes_batch, kzg_ntt per blob, kzg_commit_batch,
 * kzg_evaluate_evaluations_batch, kzg_open_batch and kzg_g1_compress per point chained by hand, 1 blob 0.87 ms (0.87-0.88) against
 * 1.45 ms (1.44-1.45); kzg_verify_blob_proofs_batch_bytes 11.9 ms (11.7-12.1) against 15.1 ms (15.0-15.2) for hashlib and
 * kzg_verify_blobs_batch_bytes at 64 blobs, and no gain at 1 blob: 10.9 ms (10.7-10.9) against 10.8 ms (10.7-10.8), one pairing
 * check either way.  Hashing the 64 blobs (8.4 MB) takes 0.57 ms on the 16 threads and 3.49 ms on one with the SHA extensions,
 * 3.13 ms and 19.9 ms in portable C++. */
int kzg_sha256(const uint8_t* data, size_t len, uint8_t out[32]);
#define KZG_SHA256_AUTO 0
#define KZG_SHA256_PORTABLE 1
#define KZG_SHA256_SHANI 2
int kzg_sha256_pieces(const uint8_t* data, size_t len, size_t piece /* > 0 */, int path, uint8_t out[32]);
int kzg_sha256_has_shani(void);
int kzg_blob_challenges_bytes(const uint8_t* blobs_be, size_t n, size_t batch, size_t stride, const uint8_t* commitments48,
                              uint8_t* out_zs_be /* batch x 32, big-endian, < r */);
int kzg_blobs_open_at_bytes(kzg_ctx* ctx, const uint8_t* blobs_be, size_t n, size_t batch, size_t stride, unsigned order,
                            const uint8_t* zs_be /* batch x 32 */, uint8_t* out_ys_be /* batch x 32 */,
                            uint8_t* out_proofs48 /* batch x 48 */);
int kzg_blobs_to_blob_proofs_bytes(kzg_ctx* ctx, const uint8_t* blobs_be, size_t n, size_t batch, size_t stride, unsigned order,
                                   const uint8_t* commitments48 /* may be NULL: computed here */,
                                   uint8_t* out_commitments48 /* may be NULL */, uint8_t* out_proofs48);
int kzg_verify_blob_proofs_batch_bytes(kzg_ctx* ctx, const uint8_t* blobs_be, size_t n, size_t batch, size_t stride, unsigned order,
                                       const uint8_t* commitments48, const uint8_t* proofs48, const void* setup_g2,
                                       size_t g2_stride_bytes, int* valid);

/* ---- device-resident / pipelined variants -------------------------------------------------
 * d_coeffs is a DEVICE pointer (n x blst_fr, Montgomery) on the context's GPU, e.g. a tensor
 * produced upstream.  submit enqueues the job of one of kzg_num_slots() slots on the context's three
 * internal HIP streams (one per phase of a job, shared by the slots) and returns at once; wait blocks
 * until that slot's job has ended, finishes the tail on the host and writes the result.  Several
 * slots in flight keep the GPU busy across the latency-bound end of each MSM. */
int kzg_num_slots(const kzg_ctx* ctx);
int kzg_commit_submit(kzg_ctx* ctx, int slot, const void* d_coeffs, size_t n);
int kzg_open_submit(kzg_ctx* ctx, int slot, const void* d_coeffs, size_t n, const uint64_t z[4],
                    const uint64_t y[4]);
int kzg_wait(kzg_ctx* ctx, int slot, uint64_t out_p1[18]);

/* Batches: `batch` polynomials of n coefficients each (polynomial p at d_coeffs + p * stride_coeffs
 * blst_fr values), committed against the same SRS in ONE pass of the kernels -- the shape of
 * BASELINE config 5 and what keeps small per-GPU shards efficient when a commitment is sharded over
 * several GPUs.  kzg_set_max_batch sizes the workspaces (default 1; it is clamped to what the sort's
 * bin table allows, read it back with kzg_max_batch).  n <= kzg_srs_len. */
int kzg_set_max_batch(kzg_ctx* ctx, size_t max_batch);
size_t kzg_max_batch(const kzg_ctx* ctx);
int kzg_commit_batch_submit(kzg_ctx* ctx, int slot, const void* d_coeffs, size_t n, size_t batch,
                            size_t stride_coeffs);
int kzg_wait_batch(kzg_ctx* ctx, int slot, uint64_t* out_p1s /* batch x 18 */, size_t batch);
/* Batched Evaluation::generate_proof (reference src/polynomial.rs:260-269): polynomial p is opened at
 * zs[p] with claimed value ys[p] (4 x uint64 Montgomery each); one quotient scan per polynomial, one
 * batched MSM over the quotients.  n >= 2, n - 1 <= kzg_srs_len.  kzg_wait_open_batch fills one status per
 * polynomial (KZG_OK, KZG_ERR_CONSTANT_POLY, KZG_ERR_REMAINDER) and the proofs of those that are KZG_OK. */
int kzg_open_batch_submit(kzg_ctx* ctx, int slot, const void* d_coeffs, size_t n, size_t batch,
                          size_t stride_coeffs, const uint64_t* zs, const uint64_t* ys);
int kzg_wait_open_batch(kzg_ctx* ctx, int slot, uint64_t* out_p1s /* batch x 18 */, int* statuses, size_t batch);

/* raw device memory helpers so a non-HIP host (Rust, Python) can stage device-resident inputs */
int kzg_dev_alloc(kzg_ctx* ctx, size_t bytes, void** out_dptr);
int kzg_dev_free(kzg_ctx* ctx, void* dptr);
int kzg_dev_upload(kzg_ctx* ctx, void* dst_dptr, const void* src_host, size_t bytes);
int kzg_dev_download(kzg_ctx* ctx, void* dst_host, const void* src_dptr, size_t bytes);

/* ---- G1 helpers on the host side of the boundary ------------------------------------------ */

/* Sum of k blst_p1 values, normalised like kzg_commit's output.  This is the "reduce" of the
 * multi-GPU MSM: each rank commits its SRS slice, the partial sums are all-gathered over RCCL and
 * every rank (or rank 0) calls this (blst_p1_add_or_double semantics, reference src/curves.rs:79-85). */
int kzg_g1_sum(const uint64_t* p1s, size_t k, uint64_t out_p1[18]);

/* ZCash 48-byte compression = what the reference's `Serialize for G1Point` emits
 * (reference src/curves.rs:99-110 -> blst_p1_compress).  The parity comparator. */
int kzg_g1_compress(const uint64_t p1[18], uint8_t out[48]);

/* Inverse: what the reference's `Deserialize for G1Point` obtains from blst_p1_uncompress +
 * blst_p1_from_affine (reference src/curves.rs:112-183), e.g. to ingest the CLI's setup.json.  On-curve
 * check only, as blst.  Next-row component. */
int kzg_g1_uncompress(const uint8_t in[48], uint64_t out_p1[18]);

/* The G2 half of SetupArtifact `index` on the host: [s^index mod r]G2 as a blst_p2 (36 x u64: x, y, z in Fp2,
 * Montgomery, z = 1), s = secret read big-endian (reference src/trusted_setup.rs:20-28, 40-53, 64-72).  A verifier
 * only ever reads index 1 (src/polynomial.rs:284): this closes the commit -> open -> verify round trip of
 * src/lib.rs:16-33 for a host that has no blst.  ~0.5 ms. */
int kzg_srs_g2_at(const uint8_t secret_be[32], uint64_t index, uint64_t out_p2[36]);

/* Evaluation::verify_proof (reference src/polynomial.rs:276-294):
 *     e(proof, [s]G2 - [z]G2) == e(commitment - [y]G1, G2)
 * commitment, proof: blst_p1; z = evaluation.point, y = evaluation.result: blst_fr (Montgomery);
 * s_g2 = setup_artifacts[1].g2: blst_p2 (36 x u64: Jacobian x, y, z in Fp2, Montgomery).  Host only (both
 * pairings in one Miller loop, ~3 ms); *valid = 1 accepted, 0 rejected.  KZG_ERR_INVALID_ARG
 * when s_g2 is not on the curve.  Next-row component. */
int kzg_verify_proof(const uint64_t commitment_p1[18], const uint64_t proof_p1[18], const uint64_t z[4],
                     const uint64_t y[4], const uint64_t s_g2_p2[36], int* valid);
/* n independent checks against the same setup (BASELINE config 5: a batch of openings and their verification),
 * spread over the host's cores; element i of every array belongs to check i (18 / 18 / 4 / 4 u64, one int). */
int kzg_verify_proof_batch(const uint64_t* commitments_p1, const uint64_t* proofs_p1, const uint64_t* zs,
                           const uint64_t* ys, const uint64_t s_g2_p2[36], size_t n, int* valid);

/* ---- powers-of-tau ceremonies: contribute to the resident SRS, verify a setup ---------- */

/* One participant's contribution: SRS[i] <- [tau^(first + i) mod r] SRS[i] for every resident point i, on the device (one
 * variable-base scalar multiplication per point; the powers are derived and split for the endomorphism there, nothing goes
 * through the host).  tau is read as kzg_srs_generate_g1 reads its secret: 32 bytes big-endian, reduced mod r; `first` has
 * the meaning it has there (the exponent of the first resident point, for a caller that holds a slice; a whole setup passes
 * 0).  Points at infinity stay at infinity.  Afterwards the window tables are rebuilt and every cache derived from the SRS
 * (FK20 transforms and comb tables, the slots' workspaces) is rebuilt or dropped as a load does it.
 *   KZG_ERR_INVALID_ARG  tau = 0 mod r (a zero contribution destroys the setup): the SRS is untouched
 *   KZG_ERR_NO_SRS       the context holds no SRS
 * The new points are produced in temporaries and copied in only after the kernels have succeeded: after a failed call the
 * context holds either the old SRS or none (kzg_srs_len = 0), never a half-updated one.  The host's copies of tau and of its
 * reduced form are wiped before the call returns; the kernel-argument copy has the lifetime of kzg_srs_generate_g1's secret
 * (it sits in the runtime's launch buffers until they are reused).  Waits for synchronous calls in flight and takes the
 * context's lock like kzg_srs_generate_g1.  A replicated multi-device context updates every device in turn (a device
 * failure in the middle leaves the devices apart: reload); a range-split one returns KZG_ERR_INVALID_ARG. */
int kzg_srs_update(kzg_ctx* ctx, const uint8_t tau_be[32], uint64_t first);

/* Is the resident SRS a setup, [s^i]G1 for one s, that matches the verifiers' [s]G2?  Every verifier of this library is
 * sound only then, and the loaders do not check it.  setup_g2 is read at indices 0 and 1 as the other verifiers read it
 * (blst_p2, g2_stride_bytes apart): [1]G2 and [s]G2.  *valid = 1 and *reason = KZG_SRS_OK, or *valid = 0 and *reason = the
 * first failure in this order (*bad_index, when given, the point it names, else (size_t)-1):
 *   KZG_SRS_G2_BAD               setup_g2[0] is not the G2 generator, or setup_g2[1] is infinity or outside the subgroup of
 *                                order r (host)
 *   KZG_SRS_INFINITY             SRS[bad_index] is the point at infinity, bad_index the least such (a setup of secret 0 is
 *                                not a setup)
 *   KZG_SRS_NOT_IN_G1            SRS[bad_index] is off the curve or outside the subgroup of order r, bad_index the least such.
 *                                The pairing of the last step cannot see this: a component of cofactor order pairs to 1
 *   KZG_SRS_FIRST_NOT_GENERATOR  only with KZG_SRS_FIRST_IS_GENERATOR in flags: SRS[0] is not [1]G1 (a slice of a setup
 *                                passes without the flag)
 *   KZG_SRS_NOT_POWERS           with rho_i uniform 128-bit from the OS CSPRNG, fresh on every call:
 *                                e(sum_{i<n-1} rho_i SRS[i+1], [1]G2) != e(sum_{i<n-1} rho_i SRS[i], [s]G2); two MSMs over the
 *                                resident tables and one two-pair check on the host.  A bad setup passes with probability
 *                                <= 2^-128; with one point there is nothing to compare
 * KZG_ERR_INVALID_ARG when a G2 point is off the twist (as the other verifiers answer it), KZG_ERR_NO_SRS without an SRS.  A
 * replicated multi-device context verifies its first device's copy; a range-split one returns KZG_ERR_INVALID_ARG. */
#define KZG_SRS_FIRST_IS_GENERATOR 1u
enum { KZG_SRS_OK = 0, KZG_SRS_G2_BAD, KZG_SRS_INFINITY, KZG_SRS_NOT_IN_G1, KZG_SRS_FIRST_NOT_GENERATOR, KZG_SRS_NOT_POWERS };
int kzg_srs_verify(kzg_ctx* ctx, const void* setup_g2, size_t g2_stride_bytes, unsigned flags, int* valid, unsigned* reason,
                   size_t* bad_index /* may be NULL */);
/* Test hook: the last step alone with the caller's weights (n - 1 blst_fr, each below r; n = kzg_srs_len): A = sum_{i<n-1}
 * rho_i SRS[i] and B = sum_{i<n-1} rho_i SRS[i+1] as normalised blst_p1, *valid = the pairing check.  No subgroup, infinity
 * or generator check runs.  n = 1: A = B = infinity, valid. */
int kzg_srs_verify_lincomb(kzg_ctx* ctx, const uint64_t* weights, const void* setup_g2, size_t g2_stride_bytes,
                           uint64_t out_a_p1[18], uint64_t out_b_p1[18], int* valid);

/* Host only, no context.  [k]Q for a blst_p2 on the twist (else KZG_ERR_INVALID_ARG), k read big-endian and reduced mod r,
 * normalised like kzg_srs_g2_at's output: a contributor makes [tau]G2 and the new [s tau]G2 with it.  The host's copies of
 * the scalar are wiped before the call returns. */
int kzg_g2_mul(const uint64_t in_p2[36], const uint8_t scalar_be[32], uint64_t out_p2[36]);
/* Host only, no context.  One link of a ceremony transcript: e(after, [1]G2) == e(before, tau_g2), where before and after
 * are SRS[1] around a contribution and tau_g2 = [tau]G2.  *valid = 0 also when before or after is infinity or off the curve,
 * or tau_g2 is infinity or outside the subgroup of order r; KZG_ERR_INVALID_ARG when tau_g2 is off the twist (as
 * kzg_verify_proof answers it). */
int kzg_srs_verify_update(const uint64_t before_p1[18], const uint64_t after_p1[18], const uint64_t tau_g2[36], int* valid);

/* ---- measurement -------------------------------------------------------------------------- */

typedef struct kzg_kernel_times {
    /* the most recent job collected from the slot.  accumulate_ms and references come from the device itself and are
     * filled for EVERY job; the other fields are HIP-event spans on the streams the kernels ran on, in milliseconds,
     * filled only for jobs submitted while timing was enabled (kzg_set_timing): a timed job records six events */
    float digits_ms;      /* scalar recoding + two-level counting sort (all of msm_sort.hip) */
    float scatter_ms;     /* queueing: buffer clears + the wait for the shared accumulation stream (not kernel cost) */
    float accumulate_ms;  /* bucket accumulation, the dominant kernel: its own duration, first wave in to last wave out on the
                           * device's constant 100 MHz clock (the kernel stamps itself; no event sits between two launches) */
    float reduce_ms;      /* finalisation + reduction trees, INCLUDING their wait behind the next accumulation */
    float quotient_ms;    /* open only: scalar-field synthetic division */
    float total_ms;       /* first kernel start -> last kernel end */
    uint64_t references;  /* non-zero scalar digits = mixed additions of the accumulation kernel (whole batch) */
    float accumulate_events_ms;  /* the HIP-event bracket around the same launch on its stream: kernel + the time it waited for the chip */
    float reserved_;
} kzg_kernel_times;

int kzg_set_timing(kzg_ctx* ctx, int enabled);
int kzg_get_times(kzg_ctx* ctx, int slot, kzg_kernel_times* out);
/* Scalar recoding chosen for the loaded SRS: recoding 0 = aligned signed windows of digit_bits
 * (table_levels = number of windows), 1 = width-digit_bits non-adjacent form over a table with one level per
 * scalar bit (table_levels = 255; chosen when that table fits the free HBM).  Any out pointer may be NULL. */
int kzg_msm_config(const kzg_ctx* ctx, int* digit_bits, int* table_levels, size_t* num_buckets, int* recoding);

#ifdef __cplusplus
}
#endif
#endif /* KZG_MI355X_H */
