// perm_quotient.cpp -- the middle rounds of a PLONK-style prover through the C-ABI (include/kzg_mi355x.h): three wire columns
// tied by a copy constraint -> kzg_permutation_commit (the accumulator z and its commitment) -> kzg_permutation_quotient (T in
// chunks of n coefficients and their commitments) -> the identity T(zeta) Z_H(zeta) = Num(zeta) at a point outside the domain,
// every polynomial evaluated by kzg_evaluate, and the chunks' commitments against kzg_commit of the chunks.
// Build:  g++ -std=c++17 -Iinclude examples/perm_quotient.cpp -Lkzg_poly_commit_exploration_amd -lkzg_mi355x -o examples/perm_quotient
// Run  :  ./examples/perm_quotient   (needs an MI355X)
#include <array>
#include <cstdio>
#include <cstring>
#include <vector>

#include "kzg_mi355x.h"

namespace {

using Fr = std::array<uint64_t, 4>;  // a blst_fr image: x 2^256 mod r
const Fr kMod = {0xffffffff00000001ULL, 0x53bda402fffe5bfeULL, 0x3339d80809a1d805ULL, 0x73eda753299d7d48ULL};
const Fr kOne = {0x00000001fffffffeULL, 0x5884b7fa00034802ULL, 0x998c4fefecbc4ff5ULL, 0x1824b159acc5056fULL};

bool geq(const Fr& a, const Fr& b) {
    for (int i = 3; i >= 0; i--)
        if (a[i] != b[i]) return a[i] > b[i];
    return true;
}
Fr sub_raw(const Fr& a, const Fr& b) {
    Fr r;
    unsigned __int128 borrow = 0;
    for (int i = 0; i < 4; i++) {
        const unsigned __int128 d = (unsigned __int128)a[i] - b[i] - (uint64_t)borrow;
        r[i] = (uint64_t)d;
        borrow = (d >> 64) & 1;
    }
    return r;
}
Fr add(const Fr& a, const Fr& b) {
    Fr s;
    unsigned __int128 c = 0;
    for (int i = 0; i < 4; i++) {
        c += (unsigned __int128)a[i] + b[i];
        s[i] = (uint64_t)c;
        c >>= 64;
    }
    return geq(s, kMod) ? sub_raw(s, kMod) : s;
}
Fr sub(const Fr& a, const Fr& b) {
    if (geq(a, b)) return sub_raw(a, b);
    Fr s;  // a + r, below 2^256
    unsigned __int128 c = 0;
    for (int i = 0; i < 4; i++) {
        c += (unsigned __int128)a[i] + kMod[i];
        s[i] = (uint64_t)c;
        c >>= 64;
    }
    return sub_raw(s, b);
}
Fr mul(const Fr& a, const Fr& b) {  // Montgomery product (CIOS)
    const uint64_t n0 = 0xfffffffeffffffffULL;
    uint64_t t[6] = {};
    for (int i = 0; i < 4; i++) {
        unsigned __int128 c = 0;
        for (int j = 0; j < 4; j++) {
            c += (unsigned __int128)a[j] * b[i] + t[j];
            t[j] = (uint64_t)c;
            c >>= 64;
        }
        c += t[4];
        t[4] = (uint64_t)c;
        t[5] = (uint64_t)(c >> 64);
        const uint64_t m = t[0] * n0;
        c = ((unsigned __int128)m * kMod[0] + t[0]) >> 64;
        for (int j = 1; j < 4; j++) {
            c += (unsigned __int128)m * kMod[j] + t[j];
            t[j - 1] = (uint64_t)c;
            c >>= 64;
        }
        c += t[4];
        t[3] = (uint64_t)c;
        t[4] = t[5] + (uint64_t)(c >> 64);
    }
    Fr r = {t[0], t[1], t[2], t[3]};
    return (t[4] || geq(r, kMod)) ? sub_raw(r, kMod) : r;
}
Fr small(unsigned v) {
    Fr r = {0, 0, 0, 0};
    for (unsigned i = 0; i < v; i++) r = add(r, kOne);
    return r;
}
Fr pow(Fr base, uint64_t e) {
    Fr acc = kOne;
    for (; e; e >>= 1, base = mul(base, base))
        if (e & 1) acc = mul(acc, base);
    return acc;
}

Fr inv(const Fr& a) {  // a^(r - 2)
    const Fr e = {kMod[0] - 2, kMod[1], kMod[2], kMod[3]};
    Fr acc = kOne;
    for (int i = 255; i >= 0; i--) {
        acc = mul(acc, acc);
        if ((e[i >> 6] >> (i & 63)) & 1) acc = mul(acc, a);
    }
    return acc;
}

#define TRY(call)                                                                                   \
    do {                                                                                            \
        const int rc_ = (call);                                                                     \
        if (rc_ != KZG_OK) {                                                                        \
            std::fprintf(stderr, "%s: %s (%s)\n", #call, kzg_strerror(rc_), kzg_last_error(ctx));   \
            return 1;                                                                               \
        }                                                                                           \
    } while (0)

}  // namespace

int main() {
    kzg_ctx* ctx = nullptr;
    if (kzg_ctx_create(0, &ctx) != KZG_OK) {
        std::fprintf(stderr, "no usable device\n");
        return 1;
    }
    const unsigned log_n = 10, log_ext = 2;
    const size_t n = (size_t)1 << log_n, t = 3, e = (size_t)1 << log_ext, N = n * e;
    uint8_t secret[32];
    for (int i = 0; i < 32; i++) secret[i] = (uint8_t)i;
    TRY(kzg_srs_generate_g1(ctx, secret, 0, n));
    Fr w;
    TRY(kzg_domain_root(log_n, w.data()));
    // row i holds one value in all three columns (a + b = c gates would constrain them; here they are simply equal), tied by the
    // permutation (j, i) -> (j + 1 mod 3, i): sigma_j[i] = k_(j+1) w^i with the coset shifts k = 1, 7, 49
    std::vector<Fr> wires(t * n), sigmas(t * n), shifts = {small(1), small(7), small(49)};
    Fr p = kOne, v = small(3);
    for (size_t i = 0; i < n; i++, p = mul(p, w), v = mul(v, small(5)))
        for (size_t j = 0; j < t; j++) {
            wires[j * n + i] = v;
            sigmas[j * n + i] = mul(shifts[(j + 1) % t], p);
        }
    // a real prover draws beta, gamma after the wire commitments, alpha after z's, zeta after T's, from its transcript
    const Fr beta = small(11), gamma = small(13), alpha = small(17), zeta = small(19);
    std::vector<Fr> z(n), T(N - n);
    Fr last;
    uint64_t z_commitment[18], chunk_commitments[3][18];
    size_t bad = 0;
    TRY(kzg_permutation_commit(ctx, wires[0].data(), sigmas[0].data(), n, t, n, shifts[0].data(), beta.data(), gamma.data(), z[0].data(),
                               last.data(), z_commitment, &bad));
    if (last != kOne) {
        std::printf("the permutation does not close\n");
        return 1;
    }
    TRY(kzg_permutation_quotient(ctx, wires[0].data(), sigmas[0].data(), z[0].data(), n, t, n, shifts[0].data(), alpha.data(), beta.data(),
                                 gamma.data(), nullptr, log_ext, T[0].data(), &chunk_commitments[0][0]));
    // the chunks' commitments are kzg_commit of the chunks
    for (size_t c = 0; c + 1 < e; c++) {
        uint64_t want[18];
        TRY(kzg_commit(ctx, T[c * n].data(), n, want));
        if (std::memcmp(want, chunk_commitments[c], sizeof want) != 0) {
            std::printf("chunk %zu: commitment differs from kzg_commit\n", c);
            return 1;
        }
    }
    // T(zeta) Z_H(zeta) = Num(zeta): every polynomial from its coefficients, by kzg_evaluate
    auto eval_values = [&](const Fr* values, const Fr& at, Fr* out) {
        std::vector<Fr> coeffs(n);
        int rc = kzg_ntt(ctx, values->data(), n, 1, coeffs[0].data());
        return rc ? rc : kzg_evaluate(ctx, coeffs[0].data(), n, at.data(), out->data());
    };
    Fr zv, zr, a, b;
    TRY(eval_values(z.data(), zeta, &zv));
    TRY(eval_values(z.data(), mul(zeta, w), &zr));
    a = zv, b = zr;
    for (size_t j = 0; j < t; j++) {
        Fr f, s;
        TRY(eval_values(&wires[j * n], zeta, &f));
        TRY(eval_values(&sigmas[j * n], zeta, &s));
        a = mul(a, add(add(f, mul(mul(beta, shifts[j]), zeta)), gamma));
        b = mul(b, add(add(f, mul(beta, s)), gamma));
    }
    const Fr zh = sub(pow(zeta, n), kOne);
    std::vector<Fr> l0_coeffs(n, inv(pow(small(2), log_n)));  // L_0 = (1 / n) (1 + X + .. + X^(n-1))
    Fr l0, Tz = {0, 0, 0, 0}, zn = kOne;
    TRY(kzg_evaluate(ctx, l0_coeffs[0].data(), n, zeta.data(), l0.data()));
    for (size_t c = 0; c + 1 < e; c++, zn = mul(zn, pow(zeta, n))) {  // T(zeta) = sum_c zeta^(c n) T_c(zeta)
        Fr y;
        TRY(kzg_evaluate(ctx, T[c * n].data(), n, zeta.data(), y.data()));
        Tz = add(Tz, mul(zn, y));
    }
    const Fr num = add(mul(alpha, sub(a, b)), mul(mul(alpha, alpha), mul(sub(zv, kOne), l0)));
    const bool ok = mul(Tz, zh) == num;
    std::printf("T(zeta) Z_H(zeta) %s Num(zeta); %zu chunk commitments equal kzg_commit\n", ok ? "==" : "!=", e - 1);
    kzg_ctx_destroy(ctx);
    return ok ? 0 : 1;
}
