// hpp_extents.cpp -- calls every wrapper of include/kzg_mi355x.hpp over tests/hpp/abi_extent_stub.cpp, on the CPU, under
// AddressSanitizer and UBSan (tests/test_hpp_extents.py builds and runs it).  The stub touches
// every byte the C header documents a call to read or write, so a buffer the header sizes short, a wrong stride or count,
// or a handle destroyed twice ends the run with a sanitizer report.  This file adds what the sanitizers cannot see: the
// size of every container a wrapper returns, and that the header's own size checks throw before the library is called.
// The shapes are those of tests/hpp/hpp_parity.cpp plus the degenerate ones (empty inputs, batch = 0, count = 0).
// With -DHPP_EXTENTS_SHORT one DIRECT call to a stub below passes a vector one element short: that build must die with
// an AddressSanitizer report, which shows the harness can fail.
#include <cstdio>
#include <cstdlib>
#include <functional>

#include "kzg_mi355x.hpp"

extern "C" void hpp_stub_print_counts(void);
extern "C" unsigned long hpp_stub_total_calls(void);
extern "C" long hpp_stub_live_circuits(void);

using namespace kzg_api;

#define CHECK(cond)                                                              \
    do {                                                                         \
        if (!(cond)) {                                                           \
            std::fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #cond); \
            std::exit(1);                                                        \
        }                                                                        \
    } while (0)

static Scalar sc(uint64_t v) {
    Scalar s;
    s.l = {v, v + 1, v + 2, 1};
    return s;
}
static std::vector<Scalar> scalars(size_t n, uint64_t seed) {
    std::vector<Scalar> v(n);
    for (size_t i = 0; i < n; i++) v[i] = sc(seed * 1000 + i + 1);
    return v;
}
using G2 = std::array<uint64_t, 36>;
// the header's own Error with `status`, thrown without a single call into the library
static void throws_before_any_call(int status, const std::function<void()>& f) {
    const unsigned long before = hpp_stub_total_calls();
    bool thrown = false;
    try {
        f();
    } catch (const Error& e) {
        thrown = e.status == status;
    }
    CHECK(thrown);
    CHECK(hpp_stub_total_calls() == before);
}
// an Error with the library's status and text
static void throws_status(int status, const std::function<void()>& f) {
    bool thrown = false;
    try {
        f();
    } catch (const Error& e) {
        thrown = e.status == status && std::string(e.what()).find(kzg_strerror(status)) == 0;
    }
    CHECK(thrown);
}

static void setup_and_polynomials(const SetupArtifacts& setup) {
    const std::array<uint8_t, 32> secret{{1, 2, 3}};
    {
        SetupArtifacts a(0);
        a.generate(secret, 16);
        CHECK(a.len() == 16);
        a.generate(secret, 16, 5);
        std::vector<G1Point> own(4);
        a.load(own.data(), sizeof(G1Point), own.size());
        CHECK(a.len() == 4);
        struct Artifact { G1Point g1; G2 g2; };  // the reference's SetupArtifact: the stride is the struct's
        std::vector<Artifact> pairs(3);
        a.load(&pairs[0].g1, sizeof(Artifact), pairs.size());
        std::vector<uint8_t> c48(48 * 7);
        a.load_compressed(c48.data(), 7);
        CHECK(a.len() == 7);
        a.save("srs.bin");
        a.load_file("srs.bin");
        CHECK(a.set_max_batch(3) == 3);
        CHECK(a.ctx() != nullptr);
        SetupArtifacts multi(std::vector<int>{0, 0}, true);
        CHECK(multi.ctx() != nullptr && multi.ctx() != a.ctx());
    }
    CHECK(SetupArtifacts::g2_at(secret).size() == 36);
    for (uint64_t j = 0; j < 3; j++) (void)SetupArtifacts::g2_at(secret, j);
    CHECK(setup.read_g1(0, 1).size() == 1);
    CHECK(setup.read_g1(3, 13).size() == 13);
    CHECK(setup.read_g1(79, 1).size() == 1);
    CHECK(setup.read_g1(0, 0).empty());

    // Scalar, G1Point
    CHECK(Scalar{}.is_zero() && !sc(1).is_zero() && sc(1) == sc(1) && !(sc(1) == sc(2)));
    G1Point g;
    CHECK(g.is_infinity());
    g.p1[12] = 1;
    CHECK(!g.is_infinity());
    CHECK(g.compress().size() == 48);
    (void)g.add(g);

    // Polynomial: trailing zeros dropped, index 0 kept
    CHECK(Polynomial::try_from({}).coefficients().empty() && Polynomial::try_from({}).degree() == 0);
    CHECK(Polynomial::try_from({Scalar{}, Scalar{}}).coefficients().size() == 1);
    std::vector<Scalar> padded = scalars(40, 1);
    for (size_t i = 31; i < 40; i++) padded[i] = Scalar{};
    CHECK(Polynomial::try_from(padded).coefficients().size() == 31 && Polynomial::try_from(padded).degree() == 30);
    const Polynomial p = Polynomial::try_from(scalars(40, 1));
    CHECK(p.degree() == 39);
    (void)p.commit(setup);
    (void)p.evaluate_at(sc(7), setup);
    (void)Polynomial::try_from({}).commit(setup);

    // batches: 3 polynomials of 40 coefficients, and the empty ones
    const std::vector<Scalar> three = scalars(120, 2);
    CHECK(commit_batch(setup, three, 40).size() == 3);
    CHECK(commit_batch(setup, {}, 40).empty());
    CHECK(commit_batch(setup, three, 0).empty());
    std::vector<int> statuses{7};
    CHECK(open_batch(setup, three, 40, scalars(3, 3), scalars(3, 4), statuses).size() == 3);
    CHECK(statuses.size() == 3 && statuses[0] == KZG_OK);
    CHECK(open_batch(setup, {}, 40, {}, {}, statuses).empty() && statuses.empty());

    const Evaluation ev{sc(5), sc(6)};
    const G1Point proof = ev.generate_proof(p, setup);
    const G2 s_g2 = SetupArtifacts::g2_at(secret, 1);
    CHECK(ev.verify_proof(proof, p.commit(setup), s_g2.data()));
}

static void domains_and_points(const SetupArtifacts& setup) {
    (void)Domain::root(6);
    for (size_t n : {(size_t)0, (size_t)1, (size_t)2, (size_t)64}) {
        CHECK(Domain::ntt(scalars(n, 5), false, setup).size() == n);
        CHECK(Domain::ntt(scalars(n, 5), true, setup).size() == n);
    }
    (void)Domain::commit(scalars(64, 6), setup);
    (void)Domain::generate_proof(scalars(64, 6), sc(1), sc(2), setup);

    const Polynomial p = Polynomial::try_from(scalars(40, 7));
    for (size_t k : {(size_t)1, (size_t)4, (size_t)5}) {
        const Evaluations ev = Evaluations::at(p, scalars(k, 8), setup);
        CHECK(ev.points.size() == k && ev.results.size() == k);
        const G1Point proof = ev.generate_proof(p, setup);
        CHECK(ev.quotient(p, setup).size() == 40 - k);  // n' - k
        CHECK(ev.verify_proof(proof, proof, std::vector<G1Point>(k), std::vector<G2>(k + 1)));
    }
    CHECK(Evaluations::at(p, {}, setup).results.empty());
    // no more coefficients than points: q = 0, nothing returned
    const Polynomial small = Polynomial::try_from(scalars(3, 9));
    CHECK(Evaluations::at(small, scalars(5, 8), setup).quotient(small, setup).empty());
    CHECK(Evaluations::at(small, scalars(3, 8), setup).quotient(small, setup).empty());

    // combined openings: 3 polynomials of 40 coefficients, and one
    const CombinedOpening co = open_combined(setup, scalars(120, 10), 40, sc(3), sc(4));
    CHECK(co.results.size() == 3);
    CHECK(verify_combined(co, std::vector<G1Point>(3), G2{}.data()));
    CHECK(open_combined(setup, scalars(40, 10), 40, sc(3), sc(4)).results.size() == 1);

    // point sets: the shape of examples/open_sets.cpp, and one where a set has a single point and comes last
    const SetsOpening so = open_sets(setup, scalars(120, 11), 40, {0, 1, 0}, {{sc(1)}, {sc(1), sc(2)}}, sc(9));
    CHECK(so.results.size() == 3 && so.results[0].size() == 1 && so.results[1].size() == 2 && so.results[2].size() == 1);
    CHECK((so.set_len() == std::vector<uint32_t>{1, 2}) && so.flat_points().size() == 3);
    CHECK(verify_sets(so, std::vector<G1Point>(3), std::vector<G1Point>(2), std::vector<G2>(3)));  // |T| = 2
    const SetsOpening so2 = open_sets(setup, scalars(80, 12), 40, {1, 0}, {{sc(1), sc(2), sc(3)}, {sc(4)}}, sc(9));
    CHECK(so2.results.size() == 2 && so2.results[0].size() == 1 && so2.results[1].size() == 3);
    CHECK((so2.set_len() == std::vector<uint32_t>{3, 1}) && so2.flat_points().size() == 4);
    CHECK(verify_sets(so2, std::vector<G1Point>(2), std::vector<G1Point>(3), std::vector<G2>(5)));  // |T| = 4
}

static void cells(const SetupArtifacts& setup) {
    const Polynomial p = Polynomial::try_from(scalars(40, 13));
    const unsigned shapes[][2] = {{6, 2}, {6, 0}, {6, 6}};
    for (const auto& s : shapes) {
        const size_t N = (size_t)1 << s[0], M = N >> s[1];
        const Cells a = Cells::of(p, s[0], s[1], setup);
        CHECK(a.values.size() == N && a.proofs.size() == M);
        const Cells b = Cells::of_evaluations(scalars(32, 14), s[0], s[1], setup);
        CHECK(b.values.size() == N && b.proofs.size() == M);
    }
    // cells longer than the domain: the library refuses the shape, the header's one-proof buffers are never written
    throws_status(KZG_ERR_INVALID_ARG, [&] { (void)Cells::of(Polynomial::try_from(scalars(5, 13)), 3, 4, setup); });
    throws_status(KZG_ERR_INVALID_ARG, [&] { (void)Cells::of_evaluations(scalars(4, 13), 3, 4, setup); });

    // quotients: n' - l coefficients per cell
    auto q = Cells::quotients(p, 6, 2, 0, 16, setup);
    CHECK(q.size() == 16);
    for (const auto& row : q) CHECK(row.size() == 36);
    q = Cells::quotients(p, 6, 2, 5, 1, setup);
    CHECK(q.size() == 1 && q[0].size() == 36);
    CHECK(Cells::quotients(p, 6, 2, 3, 0, setup).empty());
    std::vector<Scalar> padded = scalars(40, 13);
    for (size_t i = 31; i < 40; i++) padded[i] = Scalar{};
    q = Cells::quotients(Polynomial::try_from(padded), 6, 2, 0, 16, setup);
    CHECK(q.size() == 16);
    for (const auto& row : q) CHECK(row.size() == 27);
    q = Cells::quotients(Polynomial::try_from(scalars(4, 13)), 6, 2, 0, 16, setup);  // n' <= l: q = 0
    CHECK(q.size() == 16);
    for (const auto& row : q) CHECK(row.empty());

    // FK20 over ragged lengths
    std::vector<Polynomial> many{Polynomial::try_from(scalars(33, 15)), Polynomial::try_from(scalars(17, 16)),
                                 Polynomial::try_from(scalars(5, 17))};
    Cells::prepare_fk20(33, 2, setup);
    const std::vector<Cells> fk = Cells::of_many_fk20(many, 6, 2, setup);
    CHECK(fk.size() == 3);
    for (const auto& c : fk) CHECK(c.values.size() == 64 && c.proofs.size() == 16);
    CHECK(Cells::of_many_fk20({}, 6, 2, setup).empty());
    CHECK(Cells::of_many_fk20({many[2]}, 6, 6, setup)[0].proofs.size() == 1);

    // batch verification: 5 records over 2 commitments, l = 4
    const std::vector<uint32_t> idx{0, 1, 1, 0, 1}, ids{3, 0, 15, 7, 7};
    const std::vector<G2> g2(5), g2_short(4);
    CHECK(Cells::verify_batch(std::vector<G1Point>(2), idx, ids, scalars(20, 18), std::vector<G1Point>(5), 6, 2, g2, setup));
    CHECK(Cells::verify_batch({}, {}, {}, {}, {}, 6, 2, g2, setup));
    throws_before_any_call(KZG_ERR_INVALID_ARG, [&] {
        (void)Cells::verify_batch(std::vector<G1Point>(2), idx, ids, scalars(20, 18), std::vector<G1Point>(5), 6, 2, g2_short, setup);
    });
    throws_before_any_call(KZG_ERR_INVALID_ARG, [&] {
        (void)Cells::verify_batch(std::vector<G1Point>(2), idx, ids, scalars(19, 18), std::vector<G1Point>(5), 6, 2, g2, setup);
    });
    const std::vector<uint8_t> c48(96), cells_be(32 * 20), p48(48 * 5);
    for (unsigned order : {KZG_ORDER_NATURAL, KZG_ORDER_BIT_REVERSED})
        CHECK(Cells::verify_batch_bytes(c48, idx, ids, cells_be, p48, 6, 2, order, g2, setup));
    CHECK(Cells::verify_batch_bytes({}, {}, {}, {}, {}, 6, 2, KZG_ORDER_NATURAL, g2, setup));
    throws_before_any_call(KZG_ERR_INVALID_ARG, [&] {
        (void)Cells::verify_batch_bytes(c48, idx, ids, cells_be, p48, 6, 2, KZG_ORDER_NATURAL, g2_short, setup);
    });
    throws_before_any_call(KZG_ERR_INVALID_ARG, [&] {
        (void)Cells::verify_batch_bytes(std::vector<uint8_t>(95), idx, ids, cells_be, p48, 6, 2, KZG_ORDER_NATURAL, g2, setup);
    });
}

static void wire(const SetupArtifacts& setup) {
    const std::vector<G2> g2(2), g2_short(1);
    const std::vector<uint8_t> c48(96), s96(96), p144(144);
    CHECK(Wire::verify_openings(c48, {0, 1, 1}, s96, s96, p144, g2, setup));
    CHECK(Wire::verify_openings({}, {}, {}, {}, {}, g2, setup));
    throws_before_any_call(KZG_ERR_INVALID_ARG, [&] { (void)Wire::verify_openings(c48, {0, 1, 1}, s96, s96, p144, g2_short, setup); });
    throws_before_any_call(KZG_ERR_INVALID_ARG, [&] { (void)Wire::verify_openings(c48, {0, 1}, s96, s96, p144, g2, setup); });

    const std::vector<uint8_t> blobs(32 * 8 * 2), z64(64);
    std::vector<uint8_t> ys{1, 2, 3};
    CHECK(Wire::verify_blobs(blobs, 8, KZG_ORDER_NATURAL, c48, z64, c48, g2, setup));
    CHECK(Wire::verify_blobs(blobs, 8, KZG_ORDER_BIT_REVERSED, c48, z64, c48, g2, setup, &ys));
    CHECK(ys.size() == 64);
    CHECK(Wire::verify_blobs({}, 8, KZG_ORDER_NATURAL, {}, {}, {}, g2, setup, &ys));  // batch = 0
    CHECK(ys.empty());
    CHECK(Wire::verify_blobs({}, 8, KZG_ORDER_NATURAL, {}, {}, {}, g2, setup));
    throws_before_any_call(KZG_ERR_INVALID_ARG, [&] { (void)Wire::verify_blobs(blobs, 0, KZG_ORDER_NATURAL, c48, z64, c48, g2, setup); });
    throws_before_any_call(KZG_ERR_INVALID_ARG, [&] { (void)Wire::verify_blobs(blobs, 7, KZG_ORDER_NATURAL, c48, z64, c48, g2, setup); });

    for (bool subgroup : {false, true}) {
        CHECK(Wire::g1_uncompress_batch(p144, subgroup, setup).size() == 3);
        CHECK(Wire::g1_uncompress_batch({}, subgroup, setup).empty());
    }
    throws_before_any_call(KZG_ERR_INVALID_ARG, [&] { (void)Wire::g1_uncompress_batch(std::vector<uint8_t>(47), true, setup); });
    CHECK(Wire::fr_from_bytes_batch(s96, setup).size() == 3);
    CHECK(Wire::fr_from_bytes_batch({}, setup).empty());
    throws_before_any_call(KZG_ERR_INVALID_ARG, [&] { (void)Wire::fr_from_bytes_batch(std::vector<uint8_t>(33), setup); });
}

static void circuit(const SetupArtifacts& setup, size_t n, size_t t, unsigned log_ext) {
    const size_t e = (size_t)1 << log_ext, nblind = 2 * t + 3 + e - 2, LT = (e - 1) * n + t + 3;
    const std::vector<Scalar> q_lin = scalars(n * t, 20), q_mul = scalars(n, 21), q_const = scalars(n, 22), sigmas = scalars(n * t, 23),
                              shifts = scalars(t, 24), wires = scalars(n * t, 25), z = scalars(n, 26), pi = scalars(n, 27);
    const Scalar alpha = sc(1), beta = sc(2), gamma = sc(3), zeta = sc(4), v = sc(5);
    throws_before_any_call(KZG_ERR_INVALID_ARG, [&] { Circuit bad(setup, scalars(n * t - 1, 20), q_mul, q_const, sigmas, shifts, log_ext); });
    throws_before_any_call(KZG_ERR_INVALID_ARG, [&] { Circuit bad(setup, q_lin, q_mul, scalars(n + 1, 22), sigmas, shifts, log_ext); });
    // a shape the library refuses: the constructor throws the library's status, nothing is left to destroy
    throws_status(KZG_ERR_INVALID_ARG, [&] { Circuit bad(setup, scalars(n, 20), q_mul, q_const, scalars(n, 23), scalars(1, 24), log_ext); });
    CHECK(hpp_stub_live_circuits() == 0);
    {
        Circuit bare(setup, q_lin, q_mul, q_const, sigmas, shifts, log_ext, false);
        CHECK(bare.key().empty() && bare.handle() != nullptr);
        throws_before_any_call(KZG_ERR_INVALID_ARG, [&] { (void)bare.prove(wires, {}, {}); });  // no key, no transcript
    }
    CHECK(hpp_stub_live_circuits() == 0);

    Circuit c(setup, q_lin, q_mul, q_const, sigmas, shifts, log_ext);
    CHECK(c.key().size() == 2 * t + 2 && c.n() == n && c.t() == t && c.handle() != nullptr);

    // round 3: the quotient
    Circuit::Quotient q = c.quotient(wires, z, alpha, beta, gamma);
    CHECK(q.coeffs.size() == (e - 1) * n && q.commitments.size() == e - 1);
    q = c.quotient(wires, z, alpha, beta, gamma, pi, scalars(e * n, 28), false);
    CHECK(q.coeffs.size() == (e - 1) * n && q.commitments.empty());
    throws_before_any_call(KZG_ERR_INVALID_ARG, [&] { (void)c.quotient(wires, z, alpha, beta, gamma, scalars(n - 1, 27)); });
    throws_before_any_call(KZG_ERR_INVALID_ARG, [&] { (void)c.quotient(wires, z, alpha, beta, gamma, {}, scalars(e * n - 1, 28)); });
    throws_before_any_call(KZG_ERR_INVALID_ARG, [&] { (void)c.quotient(scalars(n * t + 1, 25), z, alpha, beta, gamma); });

    // round 5: open, linearise, and check_open_sizes in front of both
    Circuit::Opening o = c.open(wires, z, q.coeffs, alpha, beta, gamma, zeta, v);
    CHECK(o.evals.size() == 2 * t);
    o = c.open(wires, z, q.coeffs, alpha, beta, gamma, zeta, v, pi);
    CHECK(o.evals.size() == 2 * t);
    const auto lin = c.linearise(wires, z, q.coeffs, alpha, beta, gamma, zeta, pi);
    CHECK(lin.first.size() == 2 * t && lin.second.size() == n);
    CHECK(c.linearise(wires, z, q.coeffs, alpha, beta, gamma, zeta).second.size() == n);
    const std::vector<Scalar> wires_short = scalars(n * t - 1, 25), z_long = scalars(n + 1, 26), t_short = scalars((e - 1) * n - 1, 29),
                              pi_short = scalars(n - 1, 27);
    throws_before_any_call(KZG_ERR_INVALID_ARG, [&] { (void)c.open(wires_short, z, q.coeffs, alpha, beta, gamma, zeta, v); });
    throws_before_any_call(KZG_ERR_INVALID_ARG, [&] { (void)c.open(wires, z_long, q.coeffs, alpha, beta, gamma, zeta, v); });
    throws_before_any_call(KZG_ERR_INVALID_ARG, [&] { (void)c.open(wires, z, t_short, alpha, beta, gamma, zeta, v); });
    throws_before_any_call(KZG_ERR_INVALID_ARG, [&] { (void)c.open(wires, z, q.coeffs, alpha, beta, gamma, zeta, v, pi_short); });
    throws_before_any_call(KZG_ERR_INVALID_ARG, [&] { (void)c.linearise(wires, z, t_short, alpha, beta, gamma, zeta); });

    // resident columns and the device form (the stub's "device" memory is host memory of the documented sizes)
    const auto col = c.column_device(KZG_CIRCUIT_COL_SIGMA + 1, KZG_CIRCUIT_VALUES);
    CHECK(col.first != nullptr && col.second == n);
    CHECK(c.column_device(KZG_CIRCUIT_COL_L0, KZG_CIRCUIT_COSET).second == e * n);
    o = c.open_device(wires.data(), n, col.first, nullptr, q.coeffs.data(), alpha, beta, gamma, zeta, v);
    CHECK(o.evals.size() == 2 * t);
    o = c.open_device(wires.data(), n, z.data(), pi.data(), q.coeffs.data(), alpha, beta, gamma, zeta, v);
    CHECK(o.evals.size() == 2 * t);

    // the blinded rounds
    const std::vector<Scalar> b = c.blinders();
    CHECK(b.size() == nblind);
    CHECK(c.commit_blinded(wires, t, b.data(), 2).size() == t);
    CHECK(c.commit_blinded(z, 1, b.data() + 2 * t, 3).size() == 1);
    CHECK(c.commit_blinded({}, 0, b.data(), 2).empty());
    throws_before_any_call(KZG_ERR_INVALID_ARG, [&] { (void)c.commit_blinded(wires, t + 1, b.data(), 2); });
    Circuit::Quotient qb = c.quotient_blinded(wires, z, alpha, beta, gamma, b, pi);
    CHECK(qb.coeffs.size() == LT && qb.commitments.size() == e - 1);
    qb = c.quotient_blinded(wires, z, alpha, beta, gamma, b, {}, false);
    CHECK(qb.coeffs.size() == LT && qb.commitments.empty());
    throws_before_any_call(KZG_ERR_INVALID_ARG, [&] { (void)c.quotient_blinded(wires, z, alpha, beta, gamma, scalars(nblind - 1, 30)); });
    o = c.open_blinded(wires, z, qb.coeffs, alpha, beta, gamma, zeta, v, b, pi);
    CHECK(o.evals.size() == 2 * t);
    o = c.open_blinded(wires, z, qb.coeffs, alpha, beta, gamma, zeta, v, b);
    CHECK(o.evals.size() == 2 * t);
    throws_before_any_call(KZG_ERR_INVALID_ARG, [&] { (void)c.open_blinded(wires, z, q.coeffs, alpha, beta, gamma, zeta, v, b); });
    throws_before_any_call(KZG_ERR_INVALID_ARG, [&] { (void)c.open_blinded(wires, z, qb.coeffs, alpha, beta, gamma, zeta, v, scalars(nblind + 1, 30)); });

    // the verifier on the parts, host only
    const std::vector<G2> g2(3);
    const G1Point g1;
    const std::vector<G1Point> wire_cm(t), t_cm(e - 1);
    CHECK(Circuit::verify(c.key(), n, log_ext, shifts, wire_cm, g1, t_cm, pi, o.evals, alpha, beta, gamma, zeta, v, o.proof, g1, g2[0].data()));
    CHECK(Circuit::verify(c.key(), n, log_ext, shifts, wire_cm, g1, t_cm, {}, o.evals, alpha, beta, gamma, zeta, v, o.proof, g1, g2[0].data()));
    CHECK(Circuit::verify(c.key(), n, log_ext, shifts, wire_cm, g1, t_cm, scalars(2, 27), o.evals, alpha, beta, gamma, zeta, v, o.proof, g1,
                          g2[0].data()));
    throws_before_any_call(KZG_ERR_INVALID_ARG, [&] {
        (void)Circuit::verify(c.key(), n, log_ext, shifts, wire_cm, g1, std::vector<G1Point>(e), {}, o.evals, alpha, beta, gamma, zeta, v, o.proof, g1,
                              g2[0].data());
    });
    throws_before_any_call(KZG_ERR_INVALID_ARG, [&] {
        (void)Circuit::verify(std::vector<G1Point>(2 * t + 1), n, log_ext, shifts, wire_cm, g1, t_cm, {}, o.evals, alpha, beta, gamma, zeta, v,
                              o.proof, g1, g2[0].data());
    });

    // the proof as bytes
    const size_t bytes = 48 * (t + e + 1) + 64 * t;
    CHECK(Circuit::proof_size(t, log_ext) == bytes);
    throws_status(KZG_ERR_INVALID_ARG, [&] { (void)Circuit::proof_size(1, log_ext); });
    std::vector<uint8_t> proof = c.prove(wires, scalars(3, 27), b);
    CHECK(proof.size() == bytes);
    CHECK(c.prove(wires, {}, {}).size() == bytes);
    CHECK(c.prove(wires, pi, b).size() == bytes);
    throws_before_any_call(KZG_ERR_INVALID_ARG, [&] { (void)c.prove(wires_short, {}, b); });
    CHECK(Circuit::proof_challenges(c.key(), n, log_ext, shifts, scalars(3, 27), proof).size() == 5);
    CHECK(Circuit::proof_challenges(c.key(), n, log_ext, shifts, {}, proof).size() == 5);
    CHECK(Circuit::verify_proof(c.key(), n, log_ext, shifts, scalars(3, 27), proof, g1, g2[0].data()));
    CHECK(Circuit::verify_proof(c.key(), n, log_ext, shifts, {}, proof, g1, g2[0].data()));
    proof.pop_back();  // a proof of another length is the library's to refuse
    throws_status(KZG_ERR_INVALID_ARG, [&] { (void)Circuit::proof_challenges(c.key(), n, log_ext, shifts, {}, proof); });
    throws_status(KZG_ERR_INVALID_ARG, [&] { (void)Circuit::verify_proof(c.key(), n, log_ext, shifts, {}, proof, g1, g2[0].data()); });
    throws_before_any_call(KZG_ERR_INVALID_ARG, [&] { (void)Circuit::proof_challenges(wire_cm, n, log_ext, shifts, {}, proof); });
    throws_before_any_call(KZG_ERR_INVALID_ARG, [&] { (void)Circuit::verify_proof(wire_cm, n, log_ext, shifts, {}, proof, g1, g2[0].data()); });

    // moves: the handle travels, the old owner lets go, nothing is destroyed twice (the stub's handles are heap objects)
    CHECK(hpp_stub_live_circuits() == 1);
    const kzg_circuit* h = c.handle();
    Circuit moved(std::move(c));
    CHECK(moved.handle() == h && c.handle() == nullptr && moved.key().size() == 2 * t + 2 && moved.n() == n && moved.t() == t);
    CHECK(moved.prove(wires, {}, b).size() == bytes);
    Circuit other(setup, q_lin, q_mul, q_const, sigmas, shifts, log_ext);
    CHECK(hpp_stub_live_circuits() == 2);
    other = std::move(moved);  // destroys other's own circuit first
    CHECK(hpp_stub_live_circuits() == 1);
    CHECK(other.handle() == h && moved.handle() == nullptr);
    CHECK(other.prove(wires, {}, b).size() == bytes);
    Circuit& self = other;
    other = std::move(self);
    CHECK(other.handle() == h && hpp_stub_live_circuits() == 1);
}

int main() {
    {
        SetupArtifacts setup(0);
        const std::array<uint8_t, 32> secret{{9}};
        setup.generate(secret, 80);

        // one direct call to a stub, so that the short build below has something to be short in
        std::vector<G1Point> direct(3);
#ifdef HPP_EXTENTS_SHORT
        direct.pop_back();
        direct.shrink_to_fit();
#endif
        check(kzg_srs_read_g1(setup.ctx(), 0, 3, reinterpret_cast<uint64_t*>(direct.data())));

        setup_and_polynomials(setup);
        domains_and_points(setup);
        cells(setup);
        wire(setup);
        circuit(setup, 8, 3, 2);   // blinded with public inputs: the smallest legal shape with e = t + 1
        circuit(setup, 16, 2, 2);  // the plain shape
        CHECK(hpp_stub_live_circuits() == 0);

        // check(): the library's text, and kzg_last_error's behind a HIP status
        throws_status(KZG_ERR_DEGREE_TOO_HIGH, [&] { check(KZG_ERR_DEGREE_TOO_HIGH); });
        throws_status(KZG_ERR_HIP, [&] { check(KZG_ERR_HIP, setup.ctx()); });
        check(KZG_OK);
    }
    hpp_stub_print_counts();
    std::printf("hpp_extents ok\n");
    return 0;
}
