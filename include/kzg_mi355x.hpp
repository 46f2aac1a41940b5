// kzg_mi355x.hpp -- header-only C++ mirror of the reference's commit / open API over the C-ABI
// (include/kzg_mi355x.h).  The reference is compiled code (Rust); with no Rust toolchain in the build
// image this is the host side a C++ caller uses.  Type and method names follow the reference:
//   Scalar                  src/scalar.rs:7-8      (blst_fr memory image, Montgomery)
//   G1Point                 src/curves.rs:10-17    (blst_p1 memory image)
//   SetupArtifacts          src/trusted_setup.rs   (the G1 half of Vec<SetupArtifact>, resident on the GPU)
//   Polynomial::commit      src/polynomial.rs:200-215
//   Evaluation::generate_proof  src/polynomial.rs:260-269
// Errors are thrown as kzg::Error carrying the reference's anyhow message (kzg_strerror).
#pragma once
#include <algorithm>
#include <array>
#include <cstdint>
#include <cstring>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "kzg_mi355x.h"

namespace kzg_api {

struct Error : std::runtime_error {
    int status;
    Error(int s, const std::string& m) : std::runtime_error(m), status(s) {}
};
inline void check(int rc, const kzg_ctx* ctx = nullptr) {
    if (rc == KZG_OK) return;
    std::string m = kzg_strerror(rc);
    if (rc == KZG_ERR_HIP && ctx) m += std::string(": ") + kzg_last_error(ctx);
    throw Error(rc, m);
}

struct Scalar {  // blst_fr: 4 x u64 little-endian limbs, Montgomery form
    std::array<uint64_t, 4> l{};
    bool is_zero() const { return (l[0] | l[1] | l[2] | l[3]) == 0; }  // src/scalar.rs:221-223
    bool operator==(const Scalar& o) const { return l == o.l; }
};

struct G1Point {  // blst_p1: {x, y, z} Jacobian, Montgomery; z == 0 <=> infinity
    std::array<uint64_t, 18> p1{};
    std::array<uint8_t, 48> compress() const {  // Serialize for G1Point, src/curves.rs:99-110
        std::array<uint8_t, 48> out{};
        check(kzg_g1_compress(p1.data(), out.data()));
        return out;
    }
    bool is_infinity() const {
        uint64_t o = 0;
        for (int i = 12; i < 18; i++) o |= p1[i];
        return o == 0;
    }
    G1Point add(const G1Point& b) const {  // src/curves.rs:79-85
        uint64_t both[36];
        std::memcpy(both, p1.data(), 144);
        std::memcpy(both + 18, b.p1.data(), 144);
        G1Point r;
        check(kzg_g1_sum(both, 2, r.p1.data()));
        return r;
    }
};

class SetupArtifacts {  // owns one engine context = one GPU with the SRS resident
   public:
    explicit SetupArtifacts(int device = 0) { check(kzg_ctx_create(device, &ctx_)); }
    // one context over several devices: SRS split by point range, commit / open sharded transparently
    // replicate_srs: every device keeps the whole SRS and batches are split by polynomial (BASELINE config 5)
    explicit SetupArtifacts(const std::vector<int>& devices, bool replicate_srs = false) {
        check(kzg_ctx_create_multi_ex(devices.data(), (int)devices.size(), replicate_srs ? KZG_MULTI_REPLICATE_SRS : 0u, &ctx_));
    }
    ~SetupArtifacts() { kzg_ctx_destroy(ctx_); }
    SetupArtifacts(const SetupArtifacts&) = delete;
    SetupArtifacts& operator=(const SetupArtifacts&) = delete;
    // SetupArtifactsGenerator::new(secret).take(n), src/trusted_setup.rs:20-28, 40-62 (G1 side)
    void generate(const std::array<uint8_t, 32>& secret_be, size_t n, uint64_t first = 0) {
        check(kzg_srs_generate_g1(ctx_, secret_be.data(), first, n), ctx_);
    }
    // from the reference's own memory: &srs[0].g1, stride = sizeof(SetupArtifact)
    void load(const void* first_g1, size_t stride_bytes, size_t n) { check(kzg_srs_load_g1(ctx_, first_g1, stride_bytes, n), ctx_); }
    // the 48-byte points of the CLI's setup.json (src/curves.rs:99-183), decompressed on the device
    void load_compressed(const uint8_t* points48, size_t n) { check(kzg_srs_load_compressed(ctx_, points48, n, nullptr), ctx_); }
    void save(const std::string& path) const { check(kzg_srs_save(ctx_, path.c_str()), ctx_); }   // binary affine cache
    void load_file(const std::string& path) { check(kzg_srs_load_file(ctx_, path.c_str()), ctx_); }
    size_t len() const { return kzg_srs_len(ctx_); }
    size_t set_max_batch(size_t b) { check(kzg_set_max_batch(ctx_, b), ctx_); return kzg_max_batch(ctx_); }
    // setup_artifacts[index].g2 = [s^index]G2 (src/trusted_setup.rs:64-72), computed on the host: what verify_proof reads at index 1
    static std::array<uint64_t, 36> g2_at(const std::array<uint8_t, 32>& secret_be, uint64_t index = 1) {
        std::array<uint64_t, 36> out{};
        check(kzg_srs_g2_at(secret_be.data(), index, out.data()));
        return out;
    }
    // SRS entries [index, index + count) back as blst_p1 (Z = 1)
    std::vector<G1Point> read_g1(size_t index, size_t count) const {
        std::vector<G1Point> out(count);
        check(kzg_srs_read_g1(ctx_, index, count, reinterpret_cast<uint64_t*>(out.data())), ctx_);
        return out;
    }
    kzg_ctx* ctx() const { return ctx_; }

   private:
    kzg_ctx* ctx_ = nullptr;
};

class Polynomial {
   public:
    // TryFrom<Vec<Scalar>>, src/polynomial.rs:55-75: trailing zeros dropped, index 0 kept
    static Polynomial try_from(std::vector<Scalar> v) {
        size_t last = 0;
        for (size_t i = 0; i < v.size(); i++)
            if (!v[i].is_zero()) last = i;
        if (!v.empty()) v.resize(last + 1);
        Polynomial p;
        p.coefficients_ = std::move(v);
        return p;
    }
    uint32_t degree() const { return coefficients_.empty() ? 0 : (uint32_t)(coefficients_.size() - 1); }  // :93-98
    const std::vector<Scalar>& coefficients() const { return coefficients_; }
    G1Point commit(const SetupArtifacts& setup) const {  // :200-215
        G1Point out;
        check(kzg_commit(setup.ctx(), reinterpret_cast<const uint64_t*>(coefficients_.data()), coefficients_.size(),
                         out.p1.data()), setup.ctx());
        return out;
    }
    Scalar evaluate_at(const Scalar& x, const SetupArtifacts& setup) const {  // :112-123
        Scalar y;
        check(kzg_evaluate(setup.ctx(), reinterpret_cast<const uint64_t*>(coefficients_.data()), coefficients_.size(),
                           x.l.data(), y.l.data()), setup.ctx());
        return y;
    }

   private:
    std::vector<Scalar> coefficients_;
};

// The loop of the reference's callers over many polynomials (src/lib.rs:16-33 once per polynomial) as ONE call:
// `batch` polynomials of n coefficients each, polynomial p at coeffs[p * n ..]; on a multi-device context the
// polynomials (replicated SRS) or every polynomial's ranges (range-split SRS) spread over the GPUs.
inline std::vector<G1Point> commit_batch(const SetupArtifacts& setup, const std::vector<Scalar>& coeffs, size_t n) {
    const size_t batch = n ? coeffs.size() / n : 0;
    std::vector<G1Point> out(batch);
    check(kzg_commit_batch(setup.ctx(), reinterpret_cast<const uint64_t*>(coeffs.data()), n, batch, n,
                           reinterpret_cast<uint64_t*>(out.data())), setup.ctx());
    return out;
}
// statuses[p]: KZG_OK, KZG_ERR_CONSTANT_POLY or KZG_ERR_REMAINDER -- what generate_proof would have returned for p
inline std::vector<G1Point> open_batch(const SetupArtifacts& setup, const std::vector<Scalar>& coeffs, size_t n,
                                       const std::vector<Scalar>& points, const std::vector<Scalar>& results, std::vector<int>& statuses) {
    const size_t batch = points.size();
    std::vector<G1Point> out(batch);
    statuses.assign(batch, KZG_OK);
    check(kzg_open_batch(setup.ctx(), reinterpret_cast<const uint64_t*>(coeffs.data()), n, batch, n,
                         reinterpret_cast<const uint64_t*>(points.data()), reinterpret_cast<const uint64_t*>(results.data()),
                         reinterpret_cast<uint64_t*>(out.data()), statuses.data()), setup.ctx());
    return out;
}
static_assert(sizeof(G1Point) == 144 && sizeof(Scalar) == 32, "memory images of blst_p1 / blst_fr");

struct Evaluation {  // src/polynomial.rs:249-253
    Scalar point, result;
    G1Point generate_proof(const Polynomial& polynomial, const SetupArtifacts& setup) const {  // :260-269
        G1Point out;
        const auto& c = polynomial.coefficients();
        check(kzg_open(setup.ctx(), reinterpret_cast<const uint64_t*>(c.data()), c.size(), point.l.data(),
                       result.l.data(), out.p1.data()), setup.ctx());
        return out;
    }
    // :276-294; s_g2 = setup_artifacts[1].g2 as blst_p2 (36 x u64).  Host-side pairing check.
    bool verify_proof(const G1Point& proof, const G1Point& commitment, const uint64_t s_g2[36]) const {
        int valid = 0;
        check(kzg_verify_proof(commitment.p1.data(), proof.p1.data(), point.l.data(), result.l.data(), s_g2, &valid), nullptr);
        return valid == 1;
    }
};

// Polynomials in evaluation form over the domain {w^i} of size n = 2^k (kzg_ntt and friends; natural order:
// values[i] = P(w^i), w = Domain::root(k)).
struct Domain {
    static Scalar root(unsigned log_n) {
        Scalar w;
        check(kzg_domain_root(log_n, w.l.data()));
        return w;
    }
    // coefficients -> values (inverse = false) or values -> coefficients (inverse = true); n a power of two <= 2^22
    static std::vector<Scalar> ntt(const std::vector<Scalar>& in, bool inverse, const SetupArtifacts& setup) {
        std::vector<Scalar> out(in.size());
        check(kzg_ntt(setup.ctx(), reinterpret_cast<const uint64_t*>(in.data()), in.size(), inverse ? 1 : 0,
                      reinterpret_cast<uint64_t*>(out.data())), setup.ctx());
        return out;
    }
    // the commitment / proof of the P with these values: kzg_commit / kzg_open of the interpolated coefficients
    static G1Point commit(const std::vector<Scalar>& values, const SetupArtifacts& setup) {
        G1Point out;
        check(kzg_commit_evaluations(setup.ctx(), reinterpret_cast<const uint64_t*>(values.data()), values.size(), out.p1.data()),
              setup.ctx());
        return out;
    }
    static G1Point generate_proof(const std::vector<Scalar>& values, const Scalar& z, const Scalar& y, const SetupArtifacts& setup) {
        G1Point out;
        check(kzg_open_evaluations(setup.ctx(), reinterpret_cast<const uint64_t*>(values.data()), values.size(), z.l.data(),
                                   y.l.data(), out.p1.data()), setup.ctx());
        return out;
    }
};

// Multiproofs (kzg_open_points): one proof for P at several points.  points / results: k Scalars each.
struct Evaluations {
    std::vector<Scalar> points, results;
    // the prover's first step: results = P(points), the device scans without a quotient
    static Evaluations at(const Polynomial& polynomial, std::vector<Scalar> points, const SetupArtifacts& setup) {
        Evaluations ev{std::move(points), {}};
        ev.results.resize(ev.points.size());
        const auto& c = polynomial.coefficients();
        check(kzg_evaluate_points(setup.ctx(), reinterpret_cast<const uint64_t*>(c.data()), c.size(),
                                  reinterpret_cast<const uint64_t*>(ev.points.data()), ev.points.size(),
                                  reinterpret_cast<uint64_t*>(ev.results.data())), setup.ctx());
        return ev;
    }
    G1Point generate_proof(const Polynomial& polynomial, const SetupArtifacts& setup) const {
        G1Point out;
        const auto& c = polynomial.coefficients();
        check(kzg_open_points(setup.ctx(), reinterpret_cast<const uint64_t*>(c.data()), c.size(),
                              reinterpret_cast<const uint64_t*>(points.data()), reinterpret_cast<const uint64_t*>(results.data()),
                              points.size(), out.p1.data()), setup.ctx());
        return out;
    }
    // the quotient alone (n' - k coefficients), e.g. to check it element-wise
    std::vector<Scalar> quotient(const Polynomial& polynomial, const SetupArtifacts& setup) const {
        const auto& c = polynomial.coefficients();
        std::vector<Scalar> q(c.size() > points.size() ? c.size() - points.size() : 1);
        size_t qn = 0;
        check(kzg_quotient_points(setup.ctx(), reinterpret_cast<const uint64_t*>(c.data()), c.size(),
                                  reinterpret_cast<const uint64_t*>(points.data()), reinterpret_cast<const uint64_t*>(results.data()),
                                  points.size(), reinterpret_cast<uint64_t*>(q.data()), &qn), setup.ctx());
        q.resize(qn);
        return q;
    }
    // host-side check; g1: SRS entries [0, k) as blst_p1 (e.g. read back with kzg_srs_read_g1), g2: [s^j]G2 for j <= k
    bool verify_proof(const G1Point& proof, const G1Point& commitment, const std::vector<G1Point>& g1,
                      const std::vector<std::array<uint64_t, 36>>& g2) const {
        int valid = 0;
        check(kzg_verify_points(commitment.p1.data(), proof.p1.data(), reinterpret_cast<const uint64_t*>(points.data()),
                                reinterpret_cast<const uint64_t*>(results.data()), points.size(), g1.data(), sizeof(G1Point),
                                g2.data(), sizeof(g2[0]), &valid), nullptr);
        return valid == 1;
    }
};

// Combined openings (kzg_open_combined): `batch` polynomials of n coefficients each (polynomial i at coeffs[i * n ..], as
// commit_batch takes them) opened at one point with ONE proof, for F = sum gamma^i P_i.  gamma has to be the challenge the
// protocol draws after the commitments and the values; nothing is hashed here.
struct CombinedOpening {
    Scalar point, gamma;
    std::vector<Scalar> results;  // P_i(point)
    G1Point proof;
};
inline CombinedOpening open_combined(const SetupArtifacts& setup, const std::vector<Scalar>& coeffs, size_t n, const Scalar& point,
                                     const Scalar& gamma) {
    const size_t batch = n ? coeffs.size() / n : 0;
    CombinedOpening out{point, gamma, std::vector<Scalar>(batch), {}};
    check(kzg_open_combined(setup.ctx(), reinterpret_cast<const uint64_t*>(coeffs.data()), n, batch, n, point.l.data(),
                            gamma.l.data(), reinterpret_cast<uint64_t*>(out.results.data()), out.proof.p1.data()), setup.ctx());
    return out;
}
// host-side check against the commitments of the polynomials; s_g2 = setup_artifacts[1].g2 as blst_p2 (36 x u64)
inline bool verify_combined(const CombinedOpening& opening, const std::vector<G1Point>& commitments, const uint64_t s_g2[36]) {
    int valid = 0;
    check(kzg_verify_combined(reinterpret_cast<const uint64_t*>(commitments.data()),
                              reinterpret_cast<const uint64_t*>(opening.results.data()), commitments.size(), opening.point.l.data(),
                              opening.gamma.l.data(), opening.proof.p1.data(), s_g2, &valid), nullptr);
    return valid == 1;
}

// Openings at several point sets (kzg_open_sets): polynomial i (n coefficients at coeffs[i * n ..]) is opened on
// sets[set_of[i]], all of them with ONE proof.  results[i]: its values in the set's point order.  gamma has to be the challenge
// the protocol draws after the commitments and the values; nothing is hashed here.
struct SetsOpening {
    std::vector<uint32_t> set_of;
    std::vector<std::vector<Scalar>> sets;
    Scalar gamma;
    std::vector<std::vector<Scalar>> results;
    G1Point proof;
    std::vector<uint32_t> set_len() const {
        std::vector<uint32_t> out;
        for (const auto& s : sets) out.push_back((uint32_t)s.size());
        return out;
    }
    std::vector<Scalar> flat_points() const {
        std::vector<Scalar> out;
        for (const auto& s : sets) out.insert(out.end(), s.begin(), s.end());
        return out;
    }
};
inline SetsOpening open_sets(const SetupArtifacts& setup, const std::vector<Scalar>& coeffs, size_t n, std::vector<uint32_t> set_of,
                             std::vector<std::vector<Scalar>> sets, const Scalar& gamma) {
    SetsOpening out{std::move(set_of), std::move(sets), gamma, {}, {}};
    const std::vector<uint32_t> len = out.set_len();
    const std::vector<Scalar> zs = out.flat_points();
    size_t total = 0;
    for (uint32_t g : out.set_of) total += g < len.size() ? len[g] : 0;
    std::vector<Scalar> ys(total ? total : 1);
    check(kzg_open_sets(setup.ctx(), reinterpret_cast<const uint64_t*>(coeffs.data()), n, out.set_of.size(), n, out.set_of.data(),
                        len.data(), len.size(), reinterpret_cast<const uint64_t*>(zs.data()), gamma.l.data(),
                        reinterpret_cast<uint64_t*>(ys.data()), out.proof.p1.data()), setup.ctx());
    size_t at = 0;
    for (uint32_t g : out.set_of) {
        out.results.emplace_back(ys.begin() + at, ys.begin() + at + len[g]);
        at += len[g];
    }
    return out;
}
// host-side check against the commitments; g1: SRS entries [0, max |S_g|) (SetupArtifacts::read_g1), g2: [s^j]G2 for
// j <= |T|, T the distinct points over all sets (SetupArtifacts::g2_at)
inline bool verify_sets(const SetsOpening& opening, const std::vector<G1Point>& commitments, const std::vector<G1Point>& g1,
                        const std::vector<std::array<uint64_t, 36>>& g2) {
    const std::vector<uint32_t> len = opening.set_len();
    const std::vector<Scalar> zs = opening.flat_points();
    std::vector<Scalar> ys;
    for (const auto& row : opening.results) ys.insert(ys.end(), row.begin(), row.end());
    int valid = 0;
    check(kzg_verify_sets(reinterpret_cast<const uint64_t*>(commitments.data()), commitments.size(), opening.set_of.data(), len.data(),
                          len.size(), reinterpret_cast<const uint64_t*>(zs.data()), reinterpret_cast<const uint64_t*>(ys.data()),
                          opening.gamma.l.data(), opening.proof.p1.data(), g1.data(), sizeof(G1Point), g2.data(), sizeof(g2[0]),
                          &valid), nullptr);
    return valid == 1;
}

// Every cell of the domain of N = 2^log_domain points and its multiproof (kzg_cells_and_proofs): cell j holds the
// l = 2^log_cell values P(w_N^(j + (N/l) i)), i < l, at values[j l + i]; proofs[j] is kzg_open_points' proof for them.
struct Cells {
    std::vector<Scalar> values;
    std::vector<G1Point> proofs;
    static Cells of(const Polynomial& polynomial, unsigned log_domain, unsigned log_cell, const SetupArtifacts& setup) {
        const auto& c = polynomial.coefficients();
        Cells out = sized(log_domain, log_cell);
        check(kzg_cells_and_proofs(setup.ctx(), reinterpret_cast<const uint64_t*>(c.data()), c.size(), log_domain, log_cell,
                                   reinterpret_cast<uint64_t*>(out.values.data()), out.proofs.front().p1.data()), setup.ctx());
        return out;
    }
    // P by its values over the domain of values.size() points (a power of two <= N)
    static Cells of_evaluations(const std::vector<Scalar>& values, unsigned log_domain, unsigned log_cell, const SetupArtifacts& setup) {
        Cells out = sized(log_domain, log_cell);
        check(kzg_cells_and_proofs_evaluations(setup.ctx(), reinterpret_cast<const uint64_t*>(values.data()), values.size(),
                                               log_domain, log_cell, reinterpret_cast<uint64_t*>(out.values.data()),
                                               out.proofs.front().p1.data()), setup.ctx());
        return out;
    }
    // the quotients of cells [first_cell, first_cell + count), n' - l coefficients each, e.g. to check them element-wise
    static std::vector<std::vector<Scalar>> quotients(const Polynomial& polynomial, unsigned log_domain, unsigned log_cell,
                                                      size_t first_cell, size_t count, const SetupArtifacts& setup) {
        const auto& c = polynomial.coefficients();
        const size_t l = (size_t)1 << log_cell, stride = c.size() > l ? c.size() - l : 0;
        std::vector<Scalar> q(count * stride + 1);
        size_t qn = 0;
        check(kzg_quotient_cells(setup.ctx(), reinterpret_cast<const uint64_t*>(c.data()), c.size(), log_domain, log_cell,
                                 first_cell, count, reinterpret_cast<uint64_t*>(q.data()), &qn), setup.ctx());
        std::vector<std::vector<Scalar>> out(count);
        for (size_t j = 0; j < count; j++) out[j].assign(q.begin() + j * stride, q.begin() + j * stride + qn);
        return out;
    }

    // the same for many polynomials at once by FK20 (kzg_cells_and_proofs_fk20): every result equals of()'s for that
    // polynomial; the polynomials may differ in length (each is zero-padded to the longest)
    static std::vector<Cells> of_many_fk20(const std::vector<Polynomial>& polynomials, unsigned log_domain, unsigned log_cell,
                                           const SetupArtifacts& setup) {
        size_t n = 0;
        for (const auto& p : polynomials) n = p.coefficients().size() > n ? p.coefficients().size() : n;
        std::vector<Scalar> c(polynomials.size() * n + 1, Scalar{});
        for (size_t b = 0; b < polynomials.size(); b++)
            std::copy(polynomials[b].coefficients().begin(), polynomials[b].coefficients().end(), c.begin() + b * n);
        const size_t N = (size_t)1 << log_domain, M = log_cell <= log_domain ? N >> log_cell : 1;
        std::vector<Scalar> values(polynomials.size() * N + 1);
        std::vector<G1Point> proofs(polynomials.size() * M + 1);
        check(kzg_cells_and_proofs_fk20(setup.ctx(), reinterpret_cast<const uint64_t*>(c.data()), n, polynomials.size(), n,
                                        log_domain, log_cell, reinterpret_cast<uint64_t*>(values.data()),
                                        proofs.front().p1.data()), setup.ctx());
        std::vector<Cells> out(polynomials.size());
        for (size_t b = 0; b < polynomials.size(); b++) {
            out[b].values.assign(values.begin() + b * N, values.begin() + (b + 1) * N);
            out[b].proofs.assign(proofs.begin() + b * M, proofs.begin() + (b + 1) * M);
        }
        return out;
    }
    // kzg_verify_cells_batch: record t claims that commitments[commitment_idx[t]] opens to the l values
    // values[t l .. t l + l) on cell cell_ids[t] with proofs[t]; all records are checked at once with random weights and one
    // pairing.  setup_g2: [s^j]G2 for j <= l (SetupArtifacts::g2_at).  True when every record is valid.
    static bool verify_batch(const std::vector<G1Point>& commitments, const std::vector<uint32_t>& commitment_idx,
                             const std::vector<uint32_t>& cell_ids, const std::vector<Scalar>& values,
                             const std::vector<G1Point>& proofs, unsigned log_domain, unsigned log_cell,
                             const std::vector<std::array<uint64_t, 36>>& setup_g2, const SetupArtifacts& setup) {
        const size_t k = cell_ids.size();
        if (commitment_idx.size() != k || proofs.size() != k || values.size() != (k << log_cell) ||
            setup_g2.size() <= ((size_t)1 << log_cell))
            throw Error(KZG_ERR_INVALID_ARG, "Cells::verify_batch: one commitment index, cell id, l values and proof per record, "
                                             "and l + 1 G2 powers");
        int valid = 0;
        check(kzg_verify_cells_batch(setup.ctx(), commitments.empty() ? nullptr : commitments.front().p1.data(), commitments.size(),
                                     commitment_idx.data(), cell_ids.data(), reinterpret_cast<const uint64_t*>(values.data()),
                                     proofs.empty() ? nullptr : proofs.front().p1.data(), k, log_domain, log_cell,
                                     setup_g2.front().data(), sizeof(setup_g2.front()), &valid),
              setup.ctx());
        return valid != 0;
    }
    // kzg_verify_cells_batch_bytes: verify_batch on the records as they travel -- commitments48 / proofs48: 48-byte
    // compressed points, cells_be: k x l x 32 big-endian bytes; order: KZG_ORDER_NATURAL, or KZG_ORDER_BIT_REVERSED for cell
    // ids and values in the sampling specs' order.  The bytes are decoded on the device.
    static bool verify_batch_bytes(const std::vector<uint8_t>& commitments48, const std::vector<uint32_t>& commitment_idx,
                                   const std::vector<uint32_t>& cell_ids, const std::vector<uint8_t>& cells_be,
                                   const std::vector<uint8_t>& proofs48, unsigned log_domain, unsigned log_cell, unsigned order,
                                   const std::vector<std::array<uint64_t, 36>>& setup_g2, const SetupArtifacts& setup) {
        const size_t k = cell_ids.size();
        if (commitment_idx.size() != k || proofs48.size() != 48 * k || cells_be.size() != ((32 * k) << log_cell) ||
            commitments48.size() % 48 || setup_g2.size() <= ((size_t)1 << log_cell))
            throw Error(KZG_ERR_INVALID_ARG, "Cells::verify_batch_bytes: one commitment index, cell id, l values and proof per "
                                             "record, and l + 1 G2 powers");
        int valid = 0;
        check(kzg_verify_cells_batch_bytes(setup.ctx(), commitments48.data(), commitments48.size() / 48, commitment_idx.data(),
                                           cell_ids.data(), cells_be.data(), proofs48.data(), k, log_domain, log_cell, order,
                                           setup_g2.front().data(), sizeof(setup_g2.front()), &valid),
              setup.ctx());
        return valid != 0;
    }
    // builds the SRS-side FK20 transforms for polynomials of n coefficients now (otherwise the first call does)
    static void prepare_fk20(size_t n, unsigned log_cell, const SetupArtifacts& setup) {
        check(kzg_fk20_prepare(setup.ctx(), n, log_cell), setup.ctx());
    }

  private:
    static Cells sized(unsigned log_domain, unsigned log_cell) {
        Cells out;
        out.values.resize((size_t)1 << log_domain);
        out.proofs.resize(log_cell <= log_domain ? (size_t)1 << (log_domain - log_cell) : 1);
        return out;
    }
};

// The other verifiers on inputs as they travel (kzg_mi355x.h, "the batch verifiers on inputs as they travel").
struct Wire {
    // kzg_verify_openings_batch_bytes: record t claims that commitment commitment_idx[t] opens to ys_be[32 t ..] at zs_be[32 t ..]
    // with proofs48[48 t ..]; setup_g2: [1]G2, [s]G2
    static bool verify_openings(const std::vector<uint8_t>& commitments48, const std::vector<uint32_t>& commitment_idx,
                                const std::vector<uint8_t>& zs_be, const std::vector<uint8_t>& ys_be,
                                const std::vector<uint8_t>& proofs48, const std::vector<std::array<uint64_t, 36>>& setup_g2,
                                const SetupArtifacts& setup) {
        const size_t k = commitment_idx.size();
        if (zs_be.size() != 32 * k || ys_be.size() != 32 * k || proofs48.size() != 48 * k || commitments48.size() % 48 ||
            setup_g2.size() < 2)
            throw Error(KZG_ERR_INVALID_ARG, "Wire::verify_openings: one index, point, value and proof per record, two G2 powers");
        int valid = 0;
        check(kzg_verify_openings_batch_bytes(setup.ctx(), commitments48.data(), commitments48.size() / 48, commitment_idx.data(),
                                              zs_be.data(), ys_be.data(), proofs48.data(), k, setup_g2.front().data(),
                                              sizeof(setup_g2.front()), &valid),
              setup.ctx());
        return valid != 0;
    }
    // kzg_verify_blobs_batch_bytes: blob b (n x 32 big-endian bytes, one after the other) has commitment b and the opening
    // proof b at the challenge zs_be[32 b ..]; out_ys_be (may be null) receives the values P_b(z_b) as big-endian bytes
    static bool verify_blobs(const std::vector<uint8_t>& blobs_be, size_t n, unsigned order, const std::vector<uint8_t>& commitments48,
                             const std::vector<uint8_t>& zs_be, const std::vector<uint8_t>& proofs48,
                             const std::vector<std::array<uint64_t, 36>>& setup_g2, const SetupArtifacts& setup,
                             std::vector<uint8_t>* out_ys_be = nullptr) {
        const size_t batch = zs_be.size() / 32;
        if (!n || blobs_be.size() != 32 * n * batch || zs_be.size() % 32 || commitments48.size() != 48 * batch ||
            proofs48.size() != 48 * batch || setup_g2.size() < 2)
            throw Error(KZG_ERR_INVALID_ARG, "Wire::verify_blobs: one commitment, challenge and proof per blob of n values");
        if (out_ys_be) out_ys_be->assign(32 * batch, 0);
        int valid = 0;
        check(kzg_verify_blobs_batch_bytes(setup.ctx(), blobs_be.data(), n, batch, n, order, commitments48.data(), zs_be.data(),
                                           proofs48.data(), setup_g2.front().data(), sizeof(setup_g2.front()),
                                           out_ys_be && batch ? out_ys_be->data() : nullptr, &valid),
              setup.ctx());
        return valid != 0;
    }
    // kzg_g1_uncompress_batch / kzg_fr_from_bytes_batch: the decoders on their own
    static std::vector<G1Point> g1_uncompress_batch(const std::vector<uint8_t>& in48, bool check_subgroup, const SetupArtifacts& setup) {
        if (in48.size() % 48) throw Error(KZG_ERR_INVALID_ARG, "Wire::g1_uncompress_batch: 48 bytes per point");
        std::vector<G1Point> out(in48.size() / 48 + 1);
        check(kzg_g1_uncompress_batch(setup.ctx(), in48.data(), in48.size() / 48, check_subgroup ? 1 : 0, out.front().p1.data(), nullptr),
              setup.ctx());
        out.pop_back();
        return out;
    }
    static std::vector<Scalar> fr_from_bytes_batch(const std::vector<uint8_t>& in32_be, const SetupArtifacts& setup) {
        if (in32_be.size() % 32) throw Error(KZG_ERR_INVALID_ARG, "Wire::fr_from_bytes_batch: 32 bytes per value");
        std::vector<Scalar> out(in32_be.size() / 32 + 1);
        check(kzg_fr_from_bytes_batch(setup.ctx(), in32_be.data(), in32_be.size() / 32, reinterpret_cast<uint64_t*>(out.data()), nullptr),
              setup.ctx());
        out.pop_back();
        return out;
    }
};

// A circuit's key resident on the device (kzg_circuit_create): move-only owner of the handle.  Columns are
// n Scalars each, the t columns of q_lin / sigmas / wires back to back; the setup must outlive the circuit.
class Circuit {
   public:
    Circuit(const SetupArtifacts& setup, const std::vector<Scalar>& q_lin, const std::vector<Scalar>& q_mul,
            const std::vector<Scalar>& q_const, const std::vector<Scalar>& sigmas, const std::vector<Scalar>& shifts, unsigned log_ext,
            bool want_key = true)
        : ctx_(setup.ctx()), n_(q_mul.size()), t_(shifts.size()), log_ext_(log_ext) {
        if (q_lin.size() != n_ * t_ || sigmas.size() != n_ * t_ || q_const.size() != n_)
            throw Error(KZG_ERR_INVALID_ARG, "Circuit: t columns of n values in q_lin and sigmas, n values in q_mul and q_const");
        if (want_key) key_.resize(2 * t_ + 2);
        const auto u = [](const std::vector<Scalar>& v) { return reinterpret_cast<const uint64_t*>(v.data()); };
        const int rc = kzg_circuit_create(ctx_, u(q_lin), u(q_mul), u(q_const), u(sigmas), n_, t_, n_, u(shifts), log_ext,
                                          want_key ? reinterpret_cast<uint64_t*>(key_.data()) : nullptr, &c_);
        if (rc != KZG_OK) throw Error(rc, std::string(kzg_strerror(rc)) + ": " + kzg_last_error(ctx_));
    }
    ~Circuit() { if (c_) kzg_circuit_destroy(ctx_, c_); }
    Circuit(const Circuit&) = delete;
    Circuit& operator=(const Circuit&) = delete;
    Circuit(Circuit&& o) noexcept : ctx_(o.ctx_), c_(o.c_), n_(o.n_), t_(o.t_), log_ext_(o.log_ext_), key_(std::move(o.key_)) { o.c_ = nullptr; }
    Circuit& operator=(Circuit&& o) noexcept {
        if (this != &o) {
            if (c_) kzg_circuit_destroy(ctx_, c_);
            ctx_ = o.ctx_, c_ = o.c_, n_ = o.n_, t_ = o.t_, log_ext_ = o.log_ext_, key_ = std::move(o.key_);
            o.c_ = nullptr;
        }
        return *this;
    }
    // the commitments of q_lin[0..t), q_mul, q_const, sigma[0..t) (empty without want_key)
    const std::vector<G1Point>& key() const { return key_; }
    size_t n() const { return n_; }
    size_t t() const { return t_; }
    const kzg_circuit* handle() const { return c_; }
    struct Quotient {
        std::vector<Scalar> coeffs;       // T: (2^log_ext - 1) n coefficients
        std::vector<G1Point> commitments; // of its chunks of n coefficients
    };
    // public_inputs: empty or n values; gate_coset: empty or 2^log_ext n values of the caller's own term
    Quotient quotient(const std::vector<Scalar>& wires, const std::vector<Scalar>& z, const Scalar& alpha, const Scalar& beta,
                      const Scalar& gamma, const std::vector<Scalar>& public_inputs = {}, const std::vector<Scalar>& gate_coset = {},
                      bool want_commitments = true) const {
        const size_t e = (size_t)1 << log_ext_;
        if (wires.size() != n_ * t_ || z.size() != n_ || (!public_inputs.empty() && public_inputs.size() != n_) ||
            (!gate_coset.empty() && gate_coset.size() != e * n_))
            throw Error(KZG_ERR_INVALID_ARG, "Circuit::quotient: column sizes");
        Quotient out;
        out.coeffs.resize((e - 1) * n_);
        if (want_commitments) out.commitments.resize(e - 1);
        const auto u = [](const std::vector<Scalar>& v) { return v.empty() ? nullptr : reinterpret_cast<const uint64_t*>(v.data()); };
        const int rc = kzg_circuit_quotient(ctx_, c_, u(wires), n_, u(z), u(public_inputs), alpha.l.data(), beta.l.data(), gamma.l.data(),
                                            u(gate_coset), out.coeffs.empty() ? nullptr : reinterpret_cast<uint64_t*>(out.coeffs.data()),
                                            want_commitments ? reinterpret_cast<uint64_t*>(out.commitments.data()) : nullptr);
        if (rc != KZG_OK) throw Error(rc, std::string(kzg_strerror(rc)) + ": " + kzg_last_error(ctx_));
        return out;
    }
    // The last round: the evaluations f_j(zeta) (t), sigma_j(zeta) (t - 1), z(zeta w) in that order, and the
    // one-element proof of all of them and of the linearisation polynomial.  The challenges are the transcript's: nothing is hashed.
    struct Opening {
        std::vector<Scalar> evals;  // 2 t
        G1Point proof;
    };
    // wires, z, public_inputs as quotient() takes them; t_coeffs: Quotient::coeffs
    Opening open(const std::vector<Scalar>& wires, const std::vector<Scalar>& z, const std::vector<Scalar>& t_coeffs, const Scalar& alpha,
                 const Scalar& beta, const Scalar& gamma, const Scalar& zeta, const Scalar& v,
                 const std::vector<Scalar>& public_inputs = {}) const {
        check_open_sizes(wires, z, t_coeffs, public_inputs);
        Opening out;
        out.evals.resize(2 * t_);
        const auto u = [](const std::vector<Scalar>& x) { return x.empty() ? nullptr : reinterpret_cast<const uint64_t*>(x.data()); };
        check(kzg_circuit_open(ctx_, c_, u(wires), n_, u(z), u(public_inputs), u(t_coeffs), alpha.l.data(), beta.l.data(), gamma.l.data(),
                               zeta.l.data(), v.l.data(), reinterpret_cast<uint64_t*>(out.evals.data()),
                               reinterpret_cast<uint64_t*>(&out.proof)),
              ctx_);
        return out;
    }
    // the same on kzg_dev_alloc buffers (d_t_coeffs: what kzg_circuit_quotient_device wrote; d_public_inputs may be null)
    Opening open_device(const void* d_wires, size_t stride, const void* d_z, const void* d_public_inputs, const void* d_t_coeffs,
                        const Scalar& alpha, const Scalar& beta, const Scalar& gamma, const Scalar& zeta, const Scalar& v) const {
        Opening out;
        out.evals.resize(2 * t_);
        check(kzg_circuit_open_device(ctx_, c_, d_wires, stride, d_z, d_public_inputs, d_t_coeffs, alpha.l.data(), beta.l.data(),
                                      gamma.l.data(), zeta.l.data(), v.l.data(), reinterpret_cast<uint64_t*>(out.evals.data()),
                                      reinterpret_cast<uint64_t*>(&out.proof)),
              ctx_);
        return out;
    }
    // test hook, no SRS: (the evaluations, the n coefficients of the linearisation polynomial)
    std::pair<std::vector<Scalar>, std::vector<Scalar>> linearise(const std::vector<Scalar>& wires, const std::vector<Scalar>& z,
                                                                  const std::vector<Scalar>& t_coeffs, const Scalar& alpha,
                                                                  const Scalar& beta, const Scalar& gamma, const Scalar& zeta,
                                                                  const std::vector<Scalar>& public_inputs = {}) const {
        check_open_sizes(wires, z, t_coeffs, public_inputs);
        std::vector<Scalar> evals(2 * t_), r(n_);
        const auto u = [](const std::vector<Scalar>& x) { return x.empty() ? nullptr : reinterpret_cast<const uint64_t*>(x.data()); };
        check(kzg_circuit_linearise(ctx_, c_, u(wires), n_, u(z), u(public_inputs), u(t_coeffs), alpha.l.data(), beta.l.data(),
                                    gamma.l.data(), zeta.l.data(), reinterpret_cast<uint64_t*>(evals.data()),
                                    reinterpret_cast<uint64_t*>(r.data())),
              ctx_);
        return {evals, r};
    }
    // The blinded rounds.  blinders(): a fresh array for one proof from the OS CSPRNG -- t pairs for the
    // wires, three for z, 2^log_ext - 2 for the chunks of T.  The same array goes to every blinded call of that proof.
    std::vector<Scalar> blinders() const {
        std::vector<Scalar> b(2 * t_ + 3 + ((size_t)1 << log_ext_) - 2);
        const int rc = kzg_circuit_blinders(t_, log_ext_, reinterpret_cast<uint64_t*>(b.data()));
        if (rc != KZG_OK) throw Error(rc, kzg_strerror(rc));
        return b;
    }
    // the commitments of `k` columns of n values over H, column c blinded with nb <= 3 blinders: the wires (nb = 2), z (nb = 3)
    std::vector<G1Point> commit_blinded(const std::vector<Scalar>& evals, size_t k, const Scalar* blinders, size_t nb) const {
        if (evals.size() != n_ * k) throw Error(KZG_ERR_INVALID_ARG, "Circuit::commit_blinded: k columns of n values");
        std::vector<G1Point> out(k);
        check(kzg_commit_evaluations_blinded(ctx_, reinterpret_cast<const uint64_t*>(evals.data()), n_, k, n_,
                                             reinterpret_cast<const uint64_t*>(blinders), nb, reinterpret_cast<uint64_t*>(out.data())),
              ctx_);
        return out;
    }
    // Quotient::coeffs: the L_T = (2^log_ext - 1) n + t + 3 coefficients of T~; commitments: of its blinded chunks
    Quotient quotient_blinded(const std::vector<Scalar>& wires, const std::vector<Scalar>& z, const Scalar& alpha, const Scalar& beta,
                              const Scalar& gamma, const std::vector<Scalar>& blinders, const std::vector<Scalar>& public_inputs = {},
                              bool want_commitments = true) const {
        const size_t e = (size_t)1 << log_ext_;
        if (wires.size() != n_ * t_ || z.size() != n_ || (!public_inputs.empty() && public_inputs.size() != n_) ||
            blinders.size() != 2 * t_ + 3 + e - 2)
            throw Error(KZG_ERR_INVALID_ARG, "Circuit::quotient_blinded: column sizes");
        Quotient out;
        out.coeffs.resize((e - 1) * n_ + t_ + 3);
        if (want_commitments) out.commitments.resize(e - 1);
        const auto u = [](const std::vector<Scalar>& v) { return v.empty() ? nullptr : reinterpret_cast<const uint64_t*>(v.data()); };
        check(kzg_circuit_quotient_blinded(ctx_, c_, u(wires), n_, u(z), u(public_inputs), alpha.l.data(), beta.l.data(), gamma.l.data(),
                                           u(blinders), reinterpret_cast<uint64_t*>(out.coeffs.data()),
                                           want_commitments ? reinterpret_cast<uint64_t*>(out.commitments.data()) : nullptr),
              ctx_);
        return out;
    }
    // t_coeffs: quotient_blinded()'s coefficients; the evaluations are those of the blinded polynomials
    Opening open_blinded(const std::vector<Scalar>& wires, const std::vector<Scalar>& z, const std::vector<Scalar>& t_coeffs,
                         const Scalar& alpha, const Scalar& beta, const Scalar& gamma, const Scalar& zeta, const Scalar& v,
                         const std::vector<Scalar>& blinders, const std::vector<Scalar>& public_inputs = {}) const {
        const size_t e = (size_t)1 << log_ext_;
        if (wires.size() != n_ * t_ || z.size() != n_ || t_coeffs.size() != (e - 1) * n_ + t_ + 3 ||
            (!public_inputs.empty() && public_inputs.size() != n_) || blinders.size() != 2 * t_ + 3 + e - 2)
            throw Error(KZG_ERR_INVALID_ARG, "Circuit::open_blinded: column sizes");
        Opening out;
        out.evals.resize(2 * t_);
        const auto u = [](const std::vector<Scalar>& x) { return x.empty() ? nullptr : reinterpret_cast<const uint64_t*>(x.data()); };
        check(kzg_circuit_open_blinded(ctx_, c_, u(wires), n_, u(z), u(public_inputs), u(t_coeffs), alpha.l.data(), beta.l.data(),
                                       gamma.l.data(), zeta.l.data(), v.l.data(), u(blinders),
                                       reinterpret_cast<uint64_t*>(out.evals.data()), reinterpret_cast<uint64_t*>(&out.proof)),
              ctx_);
        return out;
    }
    // Host only, no context (kzg_circuit_verify): key as key(), the commitments of the wires, of z and of T's chunks, the public
    // inputs at rows 0 .. size - 1, Opening::evals; setup_g1: [s^0]G1; setup_g2: [s^j]G2, j <= 2 (36 u64 each, back to back)
    static bool verify(const std::vector<G1Point>& key, size_t n, unsigned log_ext, const std::vector<Scalar>& shifts,
                       const std::vector<G1Point>& wire_commitments, const G1Point& z_commitment,
                       const std::vector<G1Point>& t_commitments, const std::vector<Scalar>& public_inputs,
                       const std::vector<Scalar>& evals, const Scalar& alpha, const Scalar& beta, const Scalar& gamma, const Scalar& zeta,
                       const Scalar& v, const G1Point& proof, const G1Point& setup_g1, const uint64_t* setup_g2) {
        const size_t t = shifts.size();
        if (key.size() != 2 * t + 2 || wire_commitments.size() != t || evals.size() != 2 * t ||
            t_commitments.size() + 1 != ((size_t)1 << log_ext))
            throw Error(KZG_ERR_INVALID_ARG, "Circuit::verify: 2 t + 2 key commitments, t wires, 2 t values, 2^log_ext - 1 chunks");
        const auto p = [](const std::vector<G1Point>& x) { return reinterpret_cast<const uint64_t*>(x.data()); };
        const auto u = [](const std::vector<Scalar>& x) { return x.empty() ? nullptr : reinterpret_cast<const uint64_t*>(x.data()); };
        int valid = 0;
        const int rc = kzg_circuit_verify(p(key), n, t, log_ext, u(shifts), p(wire_commitments), reinterpret_cast<const uint64_t*>(&z_commitment),
                                          p(t_commitments), u(public_inputs), public_inputs.size(), u(evals), alpha.l.data(),
                                          beta.l.data(), gamma.l.data(), zeta.l.data(), v.l.data(),
                                          reinterpret_cast<const uint64_t*>(&proof), &setup_g1, sizeof(G1Point), setup_g2, 288, &valid);
        if (rc != KZG_OK) throw Error(rc, kzg_strerror(rc));
        return valid != 0;
    }
    // The proof in one call (kzg_circuit_prove): wires t x n values back to back, public_inputs the values of rows 0 .. size - 1
    // (may be empty), blinders empty for a plain proof (NOT zero-knowledge) or the array of kzg_circuit_blinders -> the proof bytes
    std::vector<uint8_t> prove(const std::vector<Scalar>& wires, const std::vector<Scalar>& public_inputs,
                               const std::vector<Scalar>& blinders) const {
        if (wires.size() != n_ * t_ || key_.size() != 2 * t_ + 2)
            throw Error(KZG_ERR_INVALID_ARG, "Circuit::prove: t x n wire values and the key's commitments");
        const auto u = [](const std::vector<Scalar>& x) { return x.empty() ? nullptr : reinterpret_cast<const uint64_t*>(x.data()); };
        std::vector<uint8_t> out(proof_size(t_, log_ext_));
        check(kzg_circuit_prove(ctx_, c_, reinterpret_cast<const uint64_t*>(key_.data()), u(wires), n_, u(public_inputs),
                                public_inputs.size(), u(blinders), out.data()),
              ctx_);
        return out;
    }
    // Host only, no context: the proof as bytes under the hashed transcript (kzg_circuit_proof_size, kzg_circuit_proof_challenges,
    // kzg_circuit_verify_proof).  challenges: beta, gamma, alpha, zeta, v from the bytes as they are (a prover calls it on the bytes
    // written so far); verify_proof: false also for bytes that do not decode; points are checked to lie on the curve only
    static size_t proof_size(size_t t, unsigned log_ext) {
        size_t bytes = 0;
        const int rc = kzg_circuit_proof_size(t, log_ext, &bytes);
        if (rc != KZG_OK) throw Error(rc, kzg_strerror(rc));
        return bytes;
    }
    static std::array<Scalar, 5> proof_challenges(const std::vector<G1Point>& key, size_t n, unsigned log_ext, const std::vector<Scalar>& shifts,
                                                  const std::vector<Scalar>& public_inputs, const std::vector<uint8_t>& proof) {
        if (key.size() != 2 * shifts.size() + 2) throw Error(KZG_ERR_INVALID_ARG, "Circuit::proof_challenges: 2 t + 2 key commitments");
        const auto u = [](const std::vector<Scalar>& x) { return x.empty() ? nullptr : reinterpret_cast<const uint64_t*>(x.data()); };
        std::array<Scalar, 5> out;
        const int rc = kzg_circuit_proof_challenges(reinterpret_cast<const uint64_t*>(key.data()), n, shifts.size(), log_ext, u(shifts),
                                                    u(public_inputs), public_inputs.size(), proof.data(), proof.size(),
                                                    reinterpret_cast<uint64_t*>(out.data()));
        if (rc != KZG_OK) throw Error(rc, kzg_strerror(rc));
        return out;
    }
    static bool verify_proof(const std::vector<G1Point>& key, size_t n, unsigned log_ext, const std::vector<Scalar>& shifts,
                             const std::vector<Scalar>& public_inputs, const std::vector<uint8_t>& proof, const G1Point& setup_g1,
                             const uint64_t* setup_g2) {
        if (key.size() != 2 * shifts.size() + 2) throw Error(KZG_ERR_INVALID_ARG, "Circuit::verify_proof: 2 t + 2 key commitments");
        const auto u = [](const std::vector<Scalar>& x) { return x.empty() ? nullptr : reinterpret_cast<const uint64_t*>(x.data()); };
        int valid = 0;
        const int rc = kzg_circuit_verify_proof(reinterpret_cast<const uint64_t*>(key.data()), n, shifts.size(), log_ext, u(shifts),
                                                u(public_inputs), public_inputs.size(), proof.data(), proof.size(), &setup_g1,
                                                sizeof(G1Point), setup_g2, 288, &valid);
        if (rc != KZG_OK) throw Error(rc, kzg_strerror(rc));
        return valid != 0;
    }
    // a resident column on the device, read-only: (pointer, length)
    std::pair<const void*, size_t> column_device(unsigned which, unsigned form) const {
        const void* p = nullptr;
        size_t len = 0;
        check(kzg_circuit_column_device(ctx_, c_, which, form, &p, &len), ctx_);
        return {p, len};
    }

   private:
    void check_open_sizes(const std::vector<Scalar>& wires, const std::vector<Scalar>& z, const std::vector<Scalar>& t_coeffs,
                          const std::vector<Scalar>& public_inputs) const {
        if (wires.size() != n_ * t_ || z.size() != n_ || t_coeffs.size() != (((size_t)1 << log_ext_) - 1) * n_ ||
            (!public_inputs.empty() && public_inputs.size() != n_))
            throw Error(KZG_ERR_INVALID_ARG, "Circuit: column sizes");
    }
    kzg_ctx* ctx_ = nullptr;
    kzg_circuit* c_ = nullptr;
    size_t n_ = 0, t_ = 0;
    unsigned log_ext_ = 0;
    std::vector<G1Point> key_;
};

}  // namespace kzg_api
