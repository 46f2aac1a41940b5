// open_points.cpp -- a multiproof through include/kzg_mi355x.hpp: commit -> evaluate at 4 points -> one proof for all
// four -> the host-side pairing check, then the same check with one claim changed.
// Build:  g++ -std=c++17 -Iinclude examples/open_points.cpp -Lkzg_poly_commit_exploration_amd -lkzg_mi355x -o examples/open_points
// Run  :  ./examples/open_points   (needs an MI355X)
#include <cstdio>

#include "kzg_mi355x.hpp"

int main() {
    using namespace kzg_api;
    try {
        SetupArtifacts setup(0);
        std::array<uint8_t, 32> secret{};
        for (int i = 0; i < 32; i++) secret[i] = (uint8_t)i;  // benches/polynomial_commitment.rs:17-20
        const size_t n = 1000;
        setup.generate(secret, n);
        // R mod r = Montgomery form of 1 (blst_fr); coefficients 1, 2, 3, ... as repeated sums of one
        const Scalar one{{0x00000001fffffffeULL, 0x5884b7fa00034802ULL, 0x998c4fefecbc4ff5ULL, 0x1824b159acc5056fULL}};
        const std::array<uint64_t, 4> r = {0xffffffff00000001ULL, 0x53bda402fffe5bfeULL, 0x3339d80809a1d805ULL, 0x73eda753299d7d48ULL};
        auto add = [&](const Scalar& a, const Scalar& b) {  // a + b mod r (both canonical)
            Scalar s;
            unsigned __int128 c = 0;
            for (int i = 0; i < 4; i++) {
                c += (unsigned __int128)a.l[i] + b.l[i];
                s.l[i] = (uint64_t)c;
                c >>= 64;
            }
            bool ge = true;
            for (int i = 3; i >= 0; i--)
                if (s.l[i] != r[i]) { ge = s.l[i] > r[i]; break; }
            if (ge) {
                unsigned __int128 b2 = 0;
                for (int i = 0; i < 4; i++) {
                    const unsigned __int128 d = (unsigned __int128)s.l[i] - r[i] - (uint64_t)b2;
                    s.l[i] = (uint64_t)d;
                    b2 = (d >> 64) & 1;
                }
            }
            return s;
        };
        std::vector<Scalar> coeffs(n);
        Scalar v = one;
        for (size_t i = 0; i < n; i++, v = add(v, one)) coeffs[i] = v;
        const Polynomial p = Polynomial::try_from(coeffs);
        const G1Point c = p.commit(setup);
        std::vector<Scalar> points;
        Scalar z = add(one, one);
        for (int i = 0; i < 4; i++, z = add(z, one)) points.push_back(z);  // z = 2, 3, 4, 5
        Evaluations ev = Evaluations::at(p, points, setup);
        const G1Point proof = ev.generate_proof(p, setup);
        std::vector<std::array<uint64_t, 36>> g2;
        for (uint64_t j = 0; j <= points.size(); j++) g2.push_back(SetupArtifacts::g2_at(secret, j));
        const std::vector<G1Point> g1 = setup.read_g1(0, points.size());
        const bool ok = ev.verify_proof(proof, c, g1, g2);
        ev.results[1] = add(ev.results[1], one);
        const bool tampered = ev.verify_proof(proof, c, g1, g2);
        for (auto b : proof.compress()) std::printf("%02x", b);
        std::printf("\n");
        if (!ok || tampered) {
            std::printf("multiproof check FAILED (accepted %d, tampered accepted %d)\n", ok, tampered);
            return 1;
        }
        std::printf("multiproof over %zu points verified; a changed claim is rejected\n", points.size());
    } catch (const Error& e) {
        std::fprintf(stderr, "kzg error %d: %s\n", e.status, e.what());
        return 1;
    }
    return 0;
}
