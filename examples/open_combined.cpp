// open_combined.cpp -- a combined opening through include/kzg_mi355x.hpp: commit to 3 polynomials -> open all three at one
// point with one proof -> the host-side pairing check of the combined claim, then the same check with one value changed.
// Build:  g++ -std=c++17 -Iinclude examples/open_combined.cpp -Lkzg_poly_commit_exploration_amd -lkzg_mi355x -o examples/open_combined
// Run  :  ./examples/open_combined   (needs an MI355X)
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
        std::vector<Scalar> coeffs(t * n);  // polynomial i: i n + 1, i n + 2, ...
        Scalar v = one;
        for (size_t i = 0; i < t * n; i++, v = add(v, one)) coeffs[i] = v;
        const std::vector<G1Point> commitments = commit_batch(setup, coeffs, n);
        // a real protocol draws the point after the commitments and gamma after the values, from its transcript
        const Scalar point = add(one, one), gamma = add(point, one);
        CombinedOpening opening = open_combined(setup, coeffs, n, point, gamma);
        const std::array<uint64_t, 36> s_g2 = SetupArtifacts::g2_at(secret, 1);
        const bool ok = verify_combined(opening, commitments, s_g2.data());
        opening.results[1] = add(opening.results[1], one);
        const bool tampered = verify_combined(opening, commitments, s_g2.data());
        for (auto b : opening.proof.compress()) std::printf("%02x", b);
        std::printf("\n");
        if (!ok || tampered) {
            std::printf("combined opening check FAILED (accepted %d, tampered accepted %d)\n", ok, tampered);
            return 1;
        }
        std::printf("combined opening of %zu polynomials verified; a changed value is rejected\n", t);
    } catch (const Error& e) {
        std::fprintf(stderr, "kzg error %d: %s\n", e.status, e.what());
        return 1;
    }
    return 0;
}
