// abi_extent_stub.cpp -- a CPU stand-in for the C-ABI symbols that include/kzg_mi355x.hpp calls, for the extent check of
// the header under host sanitizers (tests/test_hpp_extents.py).  No device, no library.
//
// Every stub (1) reads every input byte that include/kzg_mi355x.h documents the call to read and folds it into a volatile
// checksum, (2) writes every documented output extent in full with a fixed pattern, (3) returns KZG_OK (valid = 1, and
// the documented value where a size is an output), and counts the call.  The extents are computed from the call's own
// arguments as the C header and DESIGN.md state them, NOT from the .hpp: a wrapper that sizes a buffer one element short,
// passes a wrong stride or a wrong count makes a stub run off the buffer, which AddressSanitizer reports.  Handles are
// small heap objects, so a double destroy or a use after destroy is a finding too.  Including kzg_mi355x.h here makes a
// drift of a prototype a compile error.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "kzg_mi355x.h"

struct kzg_ctx {
    uint32_t magic = 0x6b7a6721u;
    size_t srs_len = 0, max_batch = 1;
    int live_circuits = 0;
};
struct kzg_circuit {
    kzg_ctx* ctx;
    size_t n, t;
    unsigned log_ext;
    std::vector<uint64_t> column;  // what kzg_circuit_column_device hands out: N values
};

namespace {
volatile uint64_t g_sink = 0;
std::map<std::string, unsigned long>& counts() {
    static std::map<std::string, unsigned long> c;
    return c;
}
constexpr size_t FR = 32, P1 = 144, P2 = 288;
constexpr uint8_t PATTERN = 0xA5;

void rd(const void* p, size_t bytes) {  // every byte is loaded: a short buffer is a heap-buffer-overflow READ
    const volatile uint8_t* b = static_cast<const volatile uint8_t*>(p);
    uint64_t s = 0;
    for (size_t i = 0; i < bytes; i++) s += b[i];
    g_sink = g_sink + s;
}
void rd_opt(const void* p, size_t bytes) { if (p) rd(p, bytes); }
void wr(void* p, size_t bytes) {  // every byte is stored: a short buffer is a heap-buffer-overflow WRITE
    volatile uint8_t* b = static_cast<volatile uint8_t*>(p);
    for (size_t i = 0; i < bytes; i++) b[i] = PATTERN;
}
void wr_opt(void* p, size_t bytes) { if (p) wr(p, bytes); }
// `cols` columns of `len` values, column j at base + 32 j stride bytes (the stride convention of the batch calls)
void rd_cols(const void* base, size_t cols, size_t len, size_t stride) {
    for (size_t j = 0; j < cols; j++) rd(static_cast<const uint8_t*>(base) + FR * j * stride, FR * len);
}
void rd_strided(const void* base, size_t count, size_t stride_bytes, size_t each) {
    for (size_t j = 0; j < count; j++) rd(static_cast<const uint8_t*>(base) + j * stride_bytes, each);
}
void use(const kzg_ctx* c) { g_sink = g_sink + c->magic; }  // a destroyed context is a heap-use-after-free
void use(const kzg_ctx* c, const kzg_circuit* k) {
    use(c);
    g_sink = g_sink + k->n + (k->ctx == c);
}
// n without trailing zero coefficients (the reference's truncation)
size_t trimmed(const uint64_t* c, size_t n) {
    while (n && !(c[4 * (n - 1)] | c[4 * (n - 1) + 1] | c[4 * (n - 1) + 2] | c[4 * (n - 1) + 3])) n--;
    return n;
}
size_t blinder_count(size_t t, unsigned log_ext) { return 2 * t + 3 + (((size_t)1 << log_ext) - 2); }
size_t proof_bytes(size_t t, unsigned log_ext) { return 48 * (t + ((size_t)1 << log_ext) + 1) + 64 * t; }
}  // namespace

#define HIT() (counts()[__func__]++)

extern "C" {

// for tests/hpp/hpp_extents.cpp: one "name count" line per symbol seen
void hpp_stub_print_counts(void) {
    for (const auto& kv : counts()) std::printf("called %s %lu\n", kv.first.c_str(), kv.second);
}

// all calls so far: lets the program see that a size check threw BEFORE any library call
unsigned long hpp_stub_total_calls(void) {
    unsigned long s = 0;
    for (const auto& kv : counts()) s += kv.second;
    return s;
}
// circuits created and not yet destroyed, over all contexts alive
static long g_live_circuits = 0;
long hpp_stub_live_circuits(void) { return g_live_circuits; }

/* ---- context ---- */
int kzg_ctx_create(int, kzg_ctx** out) { HIT(); *out = new kzg_ctx; return KZG_OK; }
int kzg_ctx_create_multi_ex(const int* devices, int ndev, unsigned, kzg_ctx** out) {
    HIT();
    rd(devices, sizeof(int) * (size_t)ndev);
    *out = new kzg_ctx;
    return KZG_OK;
}
void kzg_ctx_destroy(kzg_ctx* ctx) {
    HIT();
    if (!ctx) return;
    use(ctx);
    ctx->magic = 0;
    delete ctx;
}
const char* kzg_strerror(int status) {
    HIT();
    switch (status) {
        case KZG_OK: return "ok";
        case KZG_ERR_INVALID_ARG: return "invalid argument";
        default: return "stub status";
    }
}
const char* kzg_last_error(const kzg_ctx* ctx) { HIT(); use(ctx); return "stub"; }

/* ---- SRS ---- */
int kzg_srs_load_g1(kzg_ctx* ctx, const void* first_g1, size_t stride_bytes, size_t n) {
    HIT(); use(ctx);
    rd_strided(first_g1, n, stride_bytes, P1);
    ctx->srs_len = n;
    return KZG_OK;
}
int kzg_srs_generate_g1(kzg_ctx* ctx, const uint8_t secret_be[32], uint64_t, size_t n) {
    HIT(); use(ctx);
    rd(secret_be, 32);
    ctx->srs_len = n;
    return KZG_OK;
}
int kzg_srs_load_compressed(kzg_ctx* ctx, const uint8_t* compressed, size_t n, size_t* bad_index) {
    HIT(); use(ctx);
    rd(compressed, 48 * n);
    if (bad_index) *bad_index = (size_t)-1;
    ctx->srs_len = n;
    return KZG_OK;
}
int kzg_srs_save(kzg_ctx* ctx, const char* path) { HIT(); use(ctx); rd(path, std::strlen(path) + 1); return KZG_OK; }
int kzg_srs_load_file(kzg_ctx* ctx, const char* path) { HIT(); use(ctx); rd(path, std::strlen(path) + 1); return KZG_OK; }
int kzg_srs_read_g1(kzg_ctx* ctx, size_t, size_t count, uint64_t* out_p1) { HIT(); use(ctx); wr(out_p1, P1 * count); return KZG_OK; }
size_t kzg_srs_len(const kzg_ctx* ctx) { HIT(); use(ctx); return ctx->srs_len; }
int kzg_set_max_batch(kzg_ctx* ctx, size_t b) { HIT(); use(ctx); ctx->max_batch = b ? b : 1; return KZG_OK; }
size_t kzg_max_batch(const kzg_ctx* ctx) { HIT(); use(ctx); return ctx->max_batch; }
int kzg_srs_g2_at(const uint8_t secret_be[32], uint64_t, uint64_t out_p2[36]) { HIT(); rd(secret_be, 32); wr(out_p2, P2); return KZG_OK; }

/* ---- the hot path ---- */
int kzg_commit(kzg_ctx* ctx, const uint64_t* c, size_t n, uint64_t out_p1[18]) { HIT(); use(ctx); rd(c, FR * n); wr(out_p1, P1); return KZG_OK; }
int kzg_open(kzg_ctx* ctx, const uint64_t* c, size_t n, const uint64_t z[4], const uint64_t y[4], uint64_t out_p1[18]) {
    HIT(); use(ctx);
    rd(c, FR * n); rd(z, FR); rd(y, FR); wr(out_p1, P1);
    return KZG_OK;
}
int kzg_commit_batch(kzg_ctx* ctx, const uint64_t* c, size_t n, size_t batch, size_t stride, uint64_t* out_p1s) {
    HIT(); use(ctx);
    rd_cols(c, batch, n, stride);
    wr(out_p1s, P1 * batch);
    return KZG_OK;
}
int kzg_open_batch(kzg_ctx* ctx, const uint64_t* c, size_t n, size_t batch, size_t stride, const uint64_t* zs, const uint64_t* ys,
                   uint64_t* out_p1s, int* statuses) {
    HIT(); use(ctx);
    rd_cols(c, batch, n, stride);
    rd(zs, FR * batch); rd(ys, FR * batch);
    wr(out_p1s, P1 * batch);
    for (size_t p = 0; p < batch; p++) statuses[p] = KZG_OK;
    return KZG_OK;
}
int kzg_evaluate(kzg_ctx* ctx, const uint64_t* c, size_t n, const uint64_t z[4], uint64_t out_y[4]) {
    HIT(); use(ctx);
    rd(c, FR * n); rd(z, FR); wr(out_y, FR);
    return KZG_OK;
}

/* ---- multiproofs ---- */
int kzg_open_points(kzg_ctx* ctx, const uint64_t* c, size_t n, const uint64_t* zs, const uint64_t* ys, size_t k, uint64_t out_p1[18]) {
    HIT(); use(ctx);
    rd(c, FR * n); rd(zs, FR * k); rd(ys, FR * k); wr(out_p1, P1);
    return KZG_OK;
}
int kzg_quotient_points(kzg_ctx* ctx, const uint64_t* c, size_t n, const uint64_t* zs, const uint64_t* ys, size_t k, uint64_t* out_q,
                        size_t* out_qn) {
    HIT(); use(ctx);
    rd(c, FR * n); rd(zs, FR * k); rd(ys, FR * k);
    if (n > k) wr(out_q, FR * (n - k));  // room for n - k entries
    const size_t nt = trimmed(c, n);
    *out_qn = nt > k ? nt - k : 0;
    return KZG_OK;
}
int kzg_evaluate_points(kzg_ctx* ctx, const uint64_t* c, size_t n, const uint64_t* zs, size_t k, uint64_t* out_ys) {
    HIT(); use(ctx);
    rd(c, FR * n); rd(zs, FR * k); wr(out_ys, FR * k);
    return KZG_OK;
}
int kzg_verify_points(const uint64_t commitment_p1[18], const uint64_t proof_p1[18], const uint64_t* zs, const uint64_t* ys, size_t k,
                      const void* setup_g1, size_t g1_stride_bytes, const void* setup_g2, size_t g2_stride_bytes, int* valid) {
    HIT();
    rd(commitment_p1, P1); rd(proof_p1, P1); rd(zs, FR * k); rd(ys, FR * k);
    rd_strided(setup_g1, k, g1_stride_bytes, P1);      // SRS G1 entries [0, k)
    rd_strided(setup_g2, k + 1, g2_stride_bytes, P2);  // [s^j]G2, j in [0, k]
    *valid = 1;
    return KZG_OK;
}

/* ---- combined openings ---- */
int kzg_open_combined(kzg_ctx* ctx, const uint64_t* c, size_t n, size_t t, size_t stride, const uint64_t z[4], const uint64_t gamma[4],
                      uint64_t* out_ys, uint64_t out_p1[18]) {
    HIT(); use(ctx);
    rd_cols(c, t, n, stride); rd(z, FR); rd(gamma, FR);
    wr(out_ys, FR * t); wr(out_p1, P1);
    return KZG_OK;
}
int kzg_verify_combined(const uint64_t* commitments_p1, const uint64_t* ys, size_t t, const uint64_t z[4], const uint64_t gamma[4],
                        const uint64_t proof_p1[18], const uint64_t s_g2[36], int* valid) {
    HIT();
    rd(commitments_p1, P1 * t); rd(ys, FR * t); rd(z, FR); rd(gamma, FR); rd(proof_p1, P1); rd(s_g2, P2);
    *valid = 1;
    return KZG_OK;
}

/* ---- openings at several point sets ---- */
static size_t sets_values(const uint32_t* set_of, const uint32_t* set_len, size_t t, size_t m, size_t* points, size_t* longest) {
    rd(set_of, 4 * t); rd(set_len, 4 * m);
    size_t total = 0;
    *points = *longest = 0;
    for (size_t g = 0; g < m; g++) {
        *points += set_len[g];
        if (set_len[g] > *longest) *longest = set_len[g];
    }
    for (size_t i = 0; i < t; i++) total += set_len[set_of[i]];  // set_of[i] < m is the caller's to keep
    return total;
}
int kzg_open_sets(kzg_ctx* ctx, const uint64_t* c, size_t n, size_t t, size_t stride, const uint32_t* set_of, const uint32_t* set_len,
                  size_t m, const uint64_t* zs, const uint64_t gamma[4], uint64_t* out_ys, uint64_t out_p1[18]) {
    HIT(); use(ctx);
    size_t points, longest;
    const size_t total = sets_values(set_of, set_len, t, m, &points, &longest);
    rd_cols(c, t, n, stride); rd(zs, FR * points); rd(gamma, FR);
    wr(out_ys, FR * total); wr(out_p1, P1);
    return KZG_OK;
}
int kzg_verify_sets(const uint64_t* commitments_p1, size_t t, const uint32_t* set_of, const uint32_t* set_len, size_t m, const uint64_t* zs,
                    const uint64_t* ys, const uint64_t gamma[4], const uint64_t proof_p1[18], const void* setup_g1, size_t g1_stride_bytes,
                    const void* setup_g2, size_t g2_stride_bytes, int* valid) {
    HIT();
    size_t points, longest;
    const size_t total = sets_values(set_of, set_len, t, m, &points, &longest);
    rd(commitments_p1, P1 * t); rd(zs, FR * points); rd(ys, FR * total); rd(gamma, FR); rd(proof_p1, P1);
    size_t distinct = 0;  // |T|
    for (size_t i = 0; i < points; i++) {
        bool seen = false;
        for (size_t j = 0; j < i && !seen; j++) seen = !std::memcmp(zs + 4 * i, zs + 4 * j, FR);
        distinct += !seen;
    }
    rd_strided(setup_g1, longest, g1_stride_bytes, P1);       // SRS G1 entries [0, max |S_g|)
    rd_strided(setup_g2, distinct + 1, g2_stride_bytes, P2);  // [s^j]G2, j <= |T|
    *valid = 1;
    return KZG_OK;
}

/* ---- evaluation form ---- */
int kzg_domain_root(unsigned, uint64_t out_mont[4]) { HIT(); wr(out_mont, FR); return KZG_OK; }
int kzg_ntt(kzg_ctx* ctx, const uint64_t* in, size_t n, int, uint64_t* out) { HIT(); use(ctx); rd(in, FR * n); wr(out, FR * n); return KZG_OK; }
int kzg_commit_evaluations(kzg_ctx* ctx, const uint64_t* e, size_t n, uint64_t out_p1[18]) { HIT(); use(ctx); rd(e, FR * n); wr(out_p1, P1); return KZG_OK; }
int kzg_open_evaluations(kzg_ctx* ctx, const uint64_t* e, size_t n, const uint64_t z[4], const uint64_t y[4], uint64_t out_p1[18]) {
    HIT(); use(ctx);
    rd(e, FR * n); rd(z, FR); rd(y, FR); wr(out_p1, P1);
    return KZG_OK;
}

/* ---- cells ---- */
static bool cell_shape_ok(unsigned log_domain, unsigned log_cell) {
    return log_domain <= KZG_NTT_MAX_LOG && log_cell <= KZG_MAX_CELL_LOG && log_cell <= log_domain;
}
int kzg_cells_and_proofs(kzg_ctx* ctx, const uint64_t* c, size_t n, unsigned log_domain, unsigned log_cell, uint64_t* out_cells,
                         uint64_t* out_proofs) {
    HIT(); use(ctx);
    if (!cell_shape_ok(log_domain, log_cell) || n > ((size_t)1 << log_domain)) return KZG_ERR_INVALID_ARG;
    rd(c, FR * n);
    wr_opt(out_cells, FR << log_domain);
    wr(out_proofs, P1 << (log_domain - log_cell));
    return KZG_OK;
}
int kzg_cells_and_proofs_evaluations(kzg_ctx* ctx, const uint64_t* e, size_t n, unsigned log_domain, unsigned log_cell, uint64_t* out_cells,
                                     uint64_t* out_proofs) {
    HIT(); use(ctx);
    if (!cell_shape_ok(log_domain, log_cell) || n > ((size_t)1 << log_domain)) return KZG_ERR_INVALID_ARG;
    rd(e, FR * n);
    wr_opt(out_cells, FR << log_domain);
    wr(out_proofs, P1 << (log_domain - log_cell));
    return KZG_OK;
}
int kzg_quotient_cells(kzg_ctx* ctx, const uint64_t* c, size_t n, unsigned log_domain, unsigned log_cell, size_t, size_t count,
                       uint64_t* out_q, size_t* out_qn) {
    HIT(); use(ctx);
    if (!cell_shape_ok(log_domain, log_cell)) return KZG_ERR_INVALID_ARG;
    const size_t l = (size_t)1 << log_cell;
    rd(c, FR * n);
    if (n > l) wr(out_q, FR * count * (n - l));  // cell c at out_q + 4 (c - first_cell) (n - l)
    const size_t nt = trimmed(c, n);
    *out_qn = nt > l ? nt - l : 0;
    return KZG_OK;
}
int kzg_cells_and_proofs_fk20(kzg_ctx* ctx, const uint64_t* c, size_t n, size_t batch, size_t stride, unsigned log_domain, unsigned log_cell,
                              uint64_t* out_cells, uint64_t* out_proofs) {
    HIT(); use(ctx);
    if (!batch) return KZG_OK;
    if (!cell_shape_ok(log_domain, log_cell) || n > ((size_t)1 << log_domain)) return KZG_ERR_INVALID_ARG;
    rd_cols(c, batch, n, stride);
    wr_opt(out_cells, (FR * batch) << log_domain);
    wr(out_proofs, (P1 * batch) << (log_domain - log_cell));
    return KZG_OK;
}
int kzg_fk20_prepare(kzg_ctx* ctx, size_t, unsigned) { HIT(); use(ctx); return KZG_OK; }
int kzg_verify_cells_batch(kzg_ctx* ctx, const uint64_t* commitments_p1, size_t num_commitments, const uint32_t* commitment_idx,
                           const uint32_t* cell_ids, const uint64_t* cells, const uint64_t* proofs_p1, size_t k, unsigned log_domain,
                           unsigned log_cell, const void* setup_g2, size_t g2_stride_bytes, int* valid) {
    HIT(); use(ctx);
    if (!cell_shape_ok(log_domain, log_cell)) return KZG_ERR_INVALID_ARG;
    const size_t l = (size_t)1 << log_cell;
    if (num_commitments) rd(commitments_p1, P1 * num_commitments);
    if (k) { rd(commitment_idx, 4 * k); rd(cell_ids, 4 * k); rd(cells, FR * k * l); rd(proofs_p1, P1 * k); }
    rd(setup_g2, P2);                                                     // index 0: [1]G2
    rd(static_cast<const uint8_t*>(setup_g2) + l * g2_stride_bytes, P2);  // index l: [s^l]G2
    *valid = 1;
    return KZG_OK;
}

/* ---- the verifiers on inputs as they travel ---- */
int kzg_verify_cells_batch_bytes(kzg_ctx* ctx, const uint8_t* commitments48, size_t num_commitments, const uint32_t* commitment_idx,
                                 const uint32_t* cell_ids, const uint8_t* cells_be, const uint8_t* proofs48, size_t k, unsigned log_domain,
                                 unsigned log_cell, unsigned order, const void* setup_g2, size_t g2_stride_bytes, int* valid) {
    HIT(); use(ctx);
    if (!cell_shape_ok(log_domain, log_cell) || order > KZG_ORDER_BIT_REVERSED) return KZG_ERR_INVALID_ARG;
    const size_t l = (size_t)1 << log_cell;
    if (num_commitments) rd(commitments48, 48 * num_commitments);
    if (k) { rd(commitment_idx, 4 * k); rd(cell_ids, 4 * k); rd(cells_be, FR * k * l); rd(proofs48, 48 * k); }
    rd(setup_g2, P2);
    rd(static_cast<const uint8_t*>(setup_g2) + l * g2_stride_bytes, P2);
    *valid = 1;
    return KZG_OK;
}
int kzg_verify_openings_batch_bytes(kzg_ctx* ctx, const uint8_t* commitments48, size_t num_commitments, const uint32_t* commitment_idx,
                                    const uint8_t* zs_be, const uint8_t* ys_be, const uint8_t* proofs48, size_t k, const void* setup_g2,
                                    size_t g2_stride_bytes, int* valid) {
    HIT(); use(ctx);
    if (num_commitments) rd(commitments48, 48 * num_commitments);
    if (k) { rd(commitment_idx, 4 * k); rd(zs_be, FR * k); rd(ys_be, FR * k); rd(proofs48, 48 * k); }
    rd_strided(setup_g2, 2, g2_stride_bytes, P2);  // indices 0 and 1
    *valid = 1;
    return KZG_OK;
}
int kzg_verify_blobs_batch_bytes(kzg_ctx* ctx, const uint8_t* blobs_be, size_t n, size_t batch, size_t stride, unsigned order,
                                 const uint8_t* commitments48, const uint8_t* zs_be, const uint8_t* proofs48, const void* setup_g2,
                                 size_t g2_stride_bytes, uint8_t* out_ys_be, int* valid) {
    HIT(); use(ctx);
    if (order > KZG_ORDER_BIT_REVERSED) return KZG_ERR_INVALID_ARG;
    if (batch) { rd_cols(blobs_be, batch, n, stride); rd(commitments48, 48 * batch); rd(zs_be, FR * batch); rd(proofs48, 48 * batch); }
    rd_strided(setup_g2, 2, g2_stride_bytes, P2);
    wr_opt(out_ys_be, FR * batch);
    *valid = 1;
    return KZG_OK;
}
int kzg_g1_uncompress_batch(kzg_ctx* ctx, const uint8_t* in48, size_t n, int, uint64_t* out_p1, size_t* bad_index) {
    HIT(); use(ctx);
    if (n) { rd(in48, 48 * n); wr(out_p1, P1 * n); }
    if (bad_index) *bad_index = (size_t)-1;
    return KZG_OK;
}
int kzg_fr_from_bytes_batch(kzg_ctx* ctx, const uint8_t* in32_be, size_t n, uint64_t* out_fr_mont, size_t* bad_index) {
    HIT(); use(ctx);
    if (n) { rd(in32_be, FR * n); wr(out_fr_mont, FR * n); }
    if (bad_index) *bad_index = (size_t)-1;
    return KZG_OK;
}

/* ---- G1 helpers and the single-opening verifier ---- */
int kzg_g1_sum(const uint64_t* p1s, size_t k, uint64_t out_p1[18]) { HIT(); rd(p1s, P1 * k); wr(out_p1, P1); return KZG_OK; }
int kzg_g1_compress(const uint64_t p1[18], uint8_t out[48]) { HIT(); rd(p1, P1); wr(out, 48); return KZG_OK; }
int kzg_verify_proof(const uint64_t commitment_p1[18], const uint64_t proof_p1[18], const uint64_t z[4], const uint64_t y[4],
                     const uint64_t s_g2_p2[36], int* valid) {
    HIT();
    rd(commitment_p1, P1); rd(proof_p1, P1); rd(z, FR); rd(y, FR); rd(s_g2_p2, P2);
    *valid = 1;
    return KZG_OK;
}

/* ---- circuits ---- */
static bool circuit_shape_ok(size_t t, unsigned log_ext) {
    return t >= KZG_CIRCUIT_MIN_COLUMNS && t <= KZG_PQ_MAX_COLUMNS && log_ext <= KZG_PQ_MAX_LOG_EXT && t + 1 <= ((size_t)1 << log_ext);
}
int kzg_circuit_create(kzg_ctx* ctx, const uint64_t* q_lin, const uint64_t* q_mul, const uint64_t* q_const, const uint64_t* sigmas, size_t n,
                       size_t t, size_t stride, const uint64_t* shifts, unsigned log_ext, uint64_t* out_key_p1s, kzg_circuit** out) {
    HIT(); use(ctx);
    *out = nullptr;  // a failed call leaves *out NULL
    if (!circuit_shape_ok(t, log_ext) || stride < n) return KZG_ERR_INVALID_ARG;
    rd_cols(q_lin, t, n, stride); rd(q_mul, FR * n); rd(q_const, FR * n); rd_cols(sigmas, t, n, stride); rd(shifts, FR * t);
    wr_opt(out_key_p1s, P1 * (2 * t + 2));
    *out = new kzg_circuit{ctx, n, t, log_ext, std::vector<uint64_t>((n << log_ext) * 4, 0x0101010101010101ull)};
    ctx->live_circuits++;
    g_live_circuits++;
    return KZG_OK;
}
int kzg_circuit_destroy(kzg_ctx* ctx, kzg_circuit* c) {
    HIT(); use(ctx, c);
    ctx->live_circuits--;
    g_live_circuits--;
    c->n = 0;
    delete c;
    return KZG_OK;
}
int kzg_circuit_quotient(kzg_ctx* ctx, const kzg_circuit* c, const uint64_t* wires, size_t stride, const uint64_t* z,
                         const uint64_t* public_inputs, const uint64_t alpha[4], const uint64_t beta[4], const uint64_t gamma[4],
                         const uint64_t* gate_coset, uint64_t* out_coeffs, uint64_t* out_p1s) {
    HIT(); use(ctx, c);
    const size_t n = c->n, e = (size_t)1 << c->log_ext, N = e * n;
    rd_cols(wires, c->t, n, stride); rd(z, FR * n); rd_opt(public_inputs, FR * n); rd(alpha, FR); rd(beta, FR); rd(gamma, FR);
    rd_opt(gate_coset, FR * N);
    wr_opt(out_coeffs, FR * (N - n));
    wr_opt(out_p1s, P1 * (e - 1));
    return KZG_OK;
}
int kzg_circuit_column_device(kzg_ctx* ctx, const kzg_circuit* c, unsigned, unsigned form, const void** d_ptr, size_t* len) {
    HIT(); use(ctx, c);
    *d_ptr = c->column.data();
    *len = form == KZG_CIRCUIT_COSET ? c->n << c->log_ext : c->n;
    return KZG_OK;
}
static void open_inputs(const kzg_circuit* c, const void* wires, size_t stride, const void* z, const void* public_inputs, const void* t_coeffs,
                        size_t t_len, const uint64_t* const challenges[], size_t nch) {
    rd_cols(wires, c->t, c->n, stride); rd(z, FR * c->n); rd_opt(public_inputs, FR * c->n); rd(t_coeffs, FR * t_len);
    for (size_t i = 0; i < nch; i++) rd(challenges[i], FR);
}
int kzg_circuit_open(kzg_ctx* ctx, const kzg_circuit* c, const uint64_t* wires, size_t stride, const uint64_t* z, const uint64_t* public_inputs,
                     const uint64_t* t_coeffs, const uint64_t alpha[4], const uint64_t beta[4], const uint64_t gamma[4], const uint64_t zeta[4],
                     const uint64_t v[4], uint64_t* out_evals, uint64_t out_p1[18]) {
    HIT(); use(ctx, c);
    const uint64_t* ch[] = {alpha, beta, gamma, zeta, v};
    open_inputs(c, wires, stride, z, public_inputs, t_coeffs, ((c->n << c->log_ext) - c->n), ch, 5);
    wr(out_evals, FR * 2 * c->t); wr(out_p1, P1);
    return KZG_OK;
}
// the stub's "device" buffers are host memory of the documented sizes, so the same reads apply
int kzg_circuit_open_device(kzg_ctx* ctx, const kzg_circuit* c, const void* d_wires, size_t stride, const void* d_z, const void* d_public_inputs,
                            const void* d_t_coeffs, const uint64_t alpha[4], const uint64_t beta[4], const uint64_t gamma[4],
                            const uint64_t zeta[4], const uint64_t v[4], uint64_t* out_evals, uint64_t out_p1[18]) {
    HIT(); use(ctx, c);
    const uint64_t* ch[] = {alpha, beta, gamma, zeta, v};
    open_inputs(c, d_wires, stride, d_z, d_public_inputs, d_t_coeffs, ((c->n << c->log_ext) - c->n), ch, 5);
    wr(out_evals, FR * 2 * c->t); wr(out_p1, P1);
    return KZG_OK;
}
int kzg_circuit_linearise(kzg_ctx* ctx, const kzg_circuit* c, const uint64_t* wires, size_t stride, const uint64_t* z,
                          const uint64_t* public_inputs, const uint64_t* t_coeffs, const uint64_t alpha[4], const uint64_t beta[4],
                          const uint64_t gamma[4], const uint64_t zeta[4], uint64_t* out_evals, uint64_t* out_r) {
    HIT(); use(ctx, c);
    const uint64_t* ch[] = {alpha, beta, gamma, zeta};
    open_inputs(c, wires, stride, z, public_inputs, t_coeffs, ((c->n << c->log_ext) - c->n), ch, 4);
    wr(out_evals, FR * 2 * c->t); wr(out_r, FR * c->n);
    return KZG_OK;
}
static void verifier_setup(const void* setup_g1, size_t g1_stride_bytes, const void* setup_g2, size_t g2_stride_bytes) {
    rd_strided(setup_g1, 1, g1_stride_bytes, P1);  // one G1 entry
    rd_strided(setup_g2, 3, g2_stride_bytes, P2);  // [s^j]G2, j <= 2
}
int kzg_circuit_verify(const uint64_t* key_p1s, size_t n, size_t t, unsigned log_ext, const uint64_t* shifts, const uint64_t* wire_p1s,
                       const uint64_t z_p1[18], const uint64_t* t_p1s, const uint64_t* public_inputs, size_t n_public, const uint64_t* evals,
                       const uint64_t alpha[4], const uint64_t beta[4], const uint64_t gamma[4], const uint64_t zeta[4], const uint64_t v[4],
                       const uint64_t proof_p1[18], const void* setup_g1, size_t g1_stride_bytes, const void* setup_g2, size_t g2_stride_bytes,
                       int* valid) {
    HIT();
    if (!circuit_shape_ok(t, log_ext) || n_public > n) return KZG_ERR_INVALID_ARG;
    rd(key_p1s, P1 * (2 * t + 2)); rd(shifts, FR * t); rd(wire_p1s, P1 * t); rd(z_p1, P1); rd(t_p1s, P1 * (((size_t)1 << log_ext) - 1));
    if (n_public) rd(public_inputs, FR * n_public);
    rd(evals, FR * 2 * t); rd(alpha, FR); rd(beta, FR); rd(gamma, FR); rd(zeta, FR); rd(v, FR); rd(proof_p1, P1);
    verifier_setup(setup_g1, g1_stride_bytes, setup_g2, g2_stride_bytes);
    *valid = 1;
    return KZG_OK;
}
int kzg_circuit_proof_size(size_t t, unsigned log_ext, size_t* bytes) {
    HIT();
    if (!circuit_shape_ok(t, log_ext)) return KZG_ERR_INVALID_ARG;
    *bytes = proof_bytes(t, log_ext);
    return KZG_OK;
}
int kzg_circuit_proof_challenges(const uint64_t* key_p1s, size_t n, size_t t, unsigned log_ext, const uint64_t* shifts,
                                 const uint64_t* public_inputs, size_t n_public, const uint8_t* proof, size_t proof_len, uint64_t* out) {
    HIT();
    if (!circuit_shape_ok(t, log_ext) || n_public > n || proof_len != proof_bytes(t, log_ext)) return KZG_ERR_INVALID_ARG;
    rd(key_p1s, P1 * (2 * t + 2)); rd(shifts, FR * t);
    if (n_public) rd(public_inputs, FR * n_public);
    rd(proof, proof_len);
    wr(out, FR * 5);
    return KZG_OK;
}
int kzg_circuit_verify_proof(const uint64_t* key_p1s, size_t n, size_t t, unsigned log_ext, const uint64_t* shifts,
                             const uint64_t* public_inputs, size_t n_public, const uint8_t* proof, size_t proof_len, const void* setup_g1,
                             size_t g1_stride_bytes, const void* setup_g2, size_t g2_stride_bytes, int* valid) {
    HIT();
    if (!circuit_shape_ok(t, log_ext) || n_public > n || proof_len != proof_bytes(t, log_ext)) return KZG_ERR_INVALID_ARG;
    rd(key_p1s, P1 * (2 * t + 2)); rd(shifts, FR * t);
    if (n_public) rd(public_inputs, FR * n_public);
    rd(proof, proof_len);
    verifier_setup(setup_g1, g1_stride_bytes, setup_g2, g2_stride_bytes);
    *valid = 1;
    return KZG_OK;
}
int kzg_circuit_prove(kzg_ctx* ctx, const kzg_circuit* c, const uint64_t* key_p1s, const uint64_t* wires, size_t stride,
                      const uint64_t* public_inputs, size_t n_public, const uint64_t* blinders, uint8_t* out_proof) {
    HIT(); use(ctx, c);
    if (n_public > c->n) return KZG_ERR_INVALID_ARG;
    rd(key_p1s, P1 * (2 * c->t + 2)); rd_cols(wires, c->t, c->n, stride);
    if (n_public) rd(public_inputs, FR * n_public);
    rd_opt(blinders, FR * blinder_count(c->t, c->log_ext));
    wr(out_proof, proof_bytes(c->t, c->log_ext));
    return KZG_OK;
}

/* ---- blinded circuit proofs ---- */
int kzg_circuit_blinders(size_t t, unsigned log_ext, uint64_t* out) {
    HIT();
    if (!circuit_shape_ok(t, log_ext)) return KZG_ERR_INVALID_ARG;
    wr(out, FR * blinder_count(t, log_ext));
    return KZG_OK;
}
int kzg_commit_evaluations_blinded(kzg_ctx* ctx, const uint64_t* evals, size_t n, size_t k, size_t stride, const uint64_t* blinders, size_t nb,
                                   uint64_t* out_p1s) {
    HIT(); use(ctx);
    rd_cols(evals, k, n, stride);
    rd(blinders, FR * k * nb);  // column c's nb blinders at blinders + 4 c nb
    wr(out_p1s, P1 * k);
    return KZG_OK;
}
int kzg_circuit_quotient_blinded(kzg_ctx* ctx, const kzg_circuit* c, const uint64_t* wires, size_t stride, const uint64_t* z,
                                 const uint64_t* public_inputs, const uint64_t alpha[4], const uint64_t beta[4], const uint64_t gamma[4],
                                 const uint64_t* blinders, uint64_t* out_coeffs, uint64_t* out_p1s) {
    HIT(); use(ctx, c);
    const size_t n = c->n, e = (size_t)1 << c->log_ext;
    rd_cols(wires, c->t, n, stride); rd(z, FR * n); rd_opt(public_inputs, FR * n); rd(alpha, FR); rd(beta, FR); rd(gamma, FR);
    rd(blinders, FR * blinder_count(c->t, c->log_ext));
    wr_opt(out_coeffs, FR * ((e - 1) * n + c->t + 3));  // L_T
    wr_opt(out_p1s, P1 * (e - 1));
    return KZG_OK;
}
int kzg_circuit_open_blinded(kzg_ctx* ctx, const kzg_circuit* c, const uint64_t* wires, size_t stride, const uint64_t* z,
                             const uint64_t* public_inputs, const uint64_t* t_coeffs, const uint64_t alpha[4], const uint64_t beta[4],
                             const uint64_t gamma[4], const uint64_t zeta[4], const uint64_t v[4], const uint64_t* blinders,
                             uint64_t* out_evals, uint64_t out_p1[18]) {
    HIT(); use(ctx, c);
    const uint64_t* ch[] = {alpha, beta, gamma, zeta, v};
    open_inputs(c, wires, stride, z, public_inputs, t_coeffs, (((size_t)1 << c->log_ext) - 1) * c->n + c->t + 3, ch, 5);
    rd(blinders, FR * blinder_count(c->t, c->log_ext));
    wr(out_evals, FR * 2 * c->t); wr(out_p1, P1);
    return KZG_OK;
}

}  // extern "C"
