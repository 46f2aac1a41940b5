// open_sets.cpp -- an opening at several point sets through include/kzg_mi355x.hpp: commit to 3 polynomials -> open two of
// them at {z} and one at {z, z w} (the shape of PLONK's last round) with ONE proof -> the host-side pairing check, then the
// same check with one value changed.
// Build:  g++ -std=c++17 -Iinclude examples/open_sets.cpp -Lkzg_poly_commit_exploration_amd -lkzg_mi355x -o examples/open_sets
// Run  :  ./examples/open_sets   (needs an MI355X)
#include <cstdio>

#include "kzg_mi355x.hpp"

int main() {
    using namespace kzg_api;
    try {
        SetupArtifacts setup(0);
        std::array<uint8_t, 32> secret{};
        for (int i = 0; i < 32; i++) secret[i] = (uint8_t)i;  // benches/polynomial_commitment.rs:17-20
        const size_t n = 1000, t = 3;
        setup.generate(secret, n);
        // coefficients: powers of the 2^20-th root of unity (any values below r do)
        const Scalar one{{0x00000001fffffffeULL, 0x5884b7fa00034802ULL, 0x998c4fefecbc4ff5ULL, 0x1824b159acc5056fULL}};
        std::vector<Scalar> coeffs(t * n);
        for (size_t i = 0; i < t * n; i++) coeffs[i] = Domain::root(1 + (unsigned)(i % 20));
        coeffs[0] = one;
        const std::vector<G1Point> commitments = commit_batch(setup, coeffs, n);
        // a real protocol draws z after the commitments and gamma after the values, from its transcript; here z = w_8 and
        // w = w_8, so z w = w_4
        const Scalar z = Domain::root(3), zw = Domain::root(2), gamma = Domain::root(5);
        SetsOpening opening = open_sets(setup, coeffs, n, {0, 1, 0}, {{z}, {z, zw}}, gamma);
        const std::vector<G1Point> g1 = setup.read_g1(0, 2);
        std::vector<std::array<uint64_t, 36>> g2;
        for (uint64_t j = 0; j <= 2; j++) g2.push_back(SetupArtifacts::g2_at(secret, j));
        const bool ok = verify_sets(opening, commitments, g1, g2);
        opening.results[1][1] = one;
        const bool tampered = verify_sets(opening, commitments, g1, g2);
        for (auto b : opening.proof.compress()) std::printf("%02x", b);
        std::printf("\n");
        if (!ok || tampered) {
            std::printf("opening check FAILED (accepted %d, tampered accepted %d)\n", ok, tampered);
            return 1;
        }
        std::printf("ok: %zu polynomials on 2 point sets opened with one proof and verified; a changed value is rejected\n", t);
    } catch (const Error& e) {
        std::fprintf(stderr, "kzg error %d: %s\n", e.status, e.what());
        return 1;
    }
    return 0;
}
