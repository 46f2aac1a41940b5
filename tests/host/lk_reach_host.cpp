// Host replay of k_lk_fold's and k_lk_constraints' arithmetic (csrc/lookup_circuit_kernels.hip) on the unchanged csrc/fr30.hip.h,
// for tests/test_circuit_lookup.py: a stand-alone program (plain g++ -fwrapv; the header is __host__ __device__ code).  Test
// infrastructure only.
//
// It replays one row (k_lk_fold) and one coset point (k_lk_constraints) per input line in the kernels' order of products, sums and
// carry passes -- s_f and s_t by one fr30_mac per column; f = (s_f q_K) k14, T = s_t x one; F = beta + f, Tt = beta + s_t,
// D = phir - phi, E = m + (D Tt) k14, W = (E F) k14 - Tt, W += (L0 phi) ak14, G' = W a3 -- not the memory layout.
//
// stdin:   K
//          K lines:  c theta beta alpha qk l0 m phi phir f_0 .. f_(c-1) tab_0 .. tab_(c-1)
//                    (blst_fr images, 64 hex digits each; theta, beta and alpha are plain scalars' images)
// stdout:  one line of reports, then per input line f, T and G' (canonical images).  The reports: for each of the sums s (the folded
//          sums), F, Tt, D, E, W: the largest |digit 0..7| entering its carry pass as a raw sum or difference (six numbers), then the
//          largest |digit 8| leaving it (six numbers); then the largest |digit 0..7| leaving any carry pass, load or product, the
//          largest |digit 8| of any product, the largest |column| of any product (exact, saturated at 2^64 - 1).
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../kzg_poly_commit_exploration_amd/csrc/fr30.hip.h"
#include "../../kzg_poly_commit_exploration_amd/csrc/host_fr.hpp"
#include "../../kzg_poly_commit_exploration_amd/csrc/fr30_host.hpp"

using namespace kzg;

namespace {

enum Sum { kFold = 0, kF, kTt, kD, kE, kW, kSums };
enum { kRaw = 0, kTop = kSums, kNorm = 2 * kSums, kProdTop, kColumn, kReports };
uint64_t rep[kReports];
void see(int which, int64_t v) {
    const uint64_t m = v < 0 ? (uint64_t)(-v) : (uint64_t)v;
    if (m > rep[which]) rep[which] = m;
}
void digits(const Fr30& v, int top) {
    for (int i = 0; i < kR9 - 1; i++) see(kNorm, v.d[i]);
    if (top >= 0) see(top, v.d[kR9 - 1]);
}
void column(__int128 acc) {
    const __int128 m = acc < 0 ? -acc : acc;
    const uint64_t s = m > (__int128)UINT64_MAX ? UINT64_MAX : (uint64_t)m;
    if (s > rep[kColumn]) rep[kColumn] = s;
}
// fr30_mul with its columns followed in exact arithmetic; the product itself is the header's
Fr30 mul(const Fr30& a, const Fr30& b) {
    int32_t m[kR9];
    __int128 acc = 0;
    for (int k = 0; k < kR9; k++) {
        for (int i = 0; i <= k; i++) acc += (__int128)a.d[i] * b.d[k - i];
        for (int j = 0; j < k; j++) acc += (__int128)m[j] * fr30_rd(k - j);
        column(acc);
        m[k] = fr30_sext30(0u - (uint32_t)(uint64_t)acc);
        acc += m[k];
        acc >>= kR9Bits;
    }
    for (int k = kR9; k < 2 * kR9 - 1; k++) {
        for (int i = k - kR9 + 1; i < kR9; i++) acc += (__int128)a.d[i] * b.d[k - i];
        for (int j = k - kR9 + 1; j < kR9; j++) acc += (__int128)m[j] * fr30_rd(k - j);
        column(acc);
        acc = (acc + (1 << (kR9Bits - 1))) >> kR9Bits;
    }
    const Fr30 p = fr30_mul(a, b);
    digits(p, kProdTop);
    return p;
}
// sum `which` of the kernels: a + sign b digit-wise, carry-normalised; the raw digits reported in 64 bits, wrapped to 32 as the
// device would
Fr30 add(Sum which, const Fr30& a, const Fr30& b, int sign = 1) {
    Fr30 r;
    for (int i = 0; i < kR9; i++) {
        const int64_t s = (int64_t)a.d[i] + sign * (int64_t)b.d[i];
        if (i < kR9 - 1) see(kRaw + which, s);
        r.d[i] = (int32_t)(uint32_t)(uint64_t)s;
    }
    r = fr30_norm(r);
    digits(r, kTop + which);
    return r;
}
bool hex_limbs(const char* h, uint32_t l[8]) {
    if (strlen(h) != 64) return false;
    for (int w = 0; w < 8; w++) {
        uint32_t v = 0;
        for (int c = 0; c < 8; c++) {
            const char ch = h[(7 - w) * 8 + c];
            const int d = ch >= '0' && ch <= '9' ? ch - '0' : (ch >= 'a' && ch <= 'f' ? ch - 'a' + 10 : -1);
            if (d < 0) return false;
            v = (v << 4) | (uint32_t)d;
        }
        l[w] = v;
    }
    return true;
}
bool ok = true;
kzg_host::Fr read_fr() {
    char h[80];
    uint32_t l[8] = {};
    ok = ok && scanf("%79s", h) == 1 && hex_limbs(h, l);
    kzg_host::Fr w;
    memcpy(w.l, l, 32);
    return w;
}
Fr30 image_of(const kzg_host::Fr& w) {
    uint32_t l[8];
    memcpy(l, w.l, 32);
    const Fr30 v = fr30_from_limbs(l);
    digits(v, -1);
    return v;
}
Fr30 read_image() { return image_of(read_fr()); }
void print(const Fr30& v) {
    uint32_t l[8];
    fr30_to_limbs(v, l);
    for (int w = 7; w >= 0; w--) printf("%08x", l[w]);
    printf("\n");
}
kzg_host::Fr pow2(int k) {
    kzg_host::Fr v = kzg_host::kFrOne;
    for (int i = 0; i < k; i++) v = kzg_host::fr_add(v, v);
    return v;
}

constexpr int kMaxC = 7;

// sum_j col_j th_j as lk_folded: one product per carry pass
Fr30 folded(const Fr30* col, const Fr30* th, int c) {
    Fr30 s = fr30_zero();
    for (int j = 0; j < c; j++) s = add(kFold, s, mul(col[j], th[j]));
    return s;
}

}  // namespace

int main() {
    int K = 0;
    if (scanf("%d", &K) != 1 || K < 1 || K > 4096) return 2;
    std::vector<Fr30> out;
    for (int k = 0; k < K; k++) {
        int c = 0;
        if (scanf("%d", &c) != 1 || c < 1 || c > kMaxC) return 2;
        const kzg_host::Fr theta = read_fr(), beta_fr = read_fr(), alpha = read_fr();
        const Fr30 qk = read_image(), l0 = read_image(), m = read_image(), phi = read_image(), phir = read_image();
        Fr30 f[kMaxC], tab[kMaxC], th[kMaxC];
        for (int j = 0; j < c; j++) f[j] = read_image();
        for (int j = 0; j < c; j++) tab[j] = read_image();
        if (!ok) return 2;
        // as LkKernelScalars (api.hip) prepares them
        kzg_host::Fr p = kzg_host::kFrOne;
        for (int j = 0; j < c; j++) {
            th[j] = fr30_arg_from_mont256(p);
            p = kzg_host::fr_mul(p, theta);
        }
        const Fr30 beta = image_of(beta_fr);
        const Fr30 k14 = fr30_arg_from_mont256(pow2(14));
        const Fr30 ak14 = fr30_arg_from_mont256(kzg_host::fr_mul(alpha, pow2(14)));
        const Fr30 a3 = fr30_arg_from_mont256(kzg_host::fr_mul(kzg_host::fr_mul(alpha, alpha), alpha));
        // k_lk_fold
        const Fr30 sf = folded(f, th, c), st = folded(tab, th, c);
        const Fr30 fq = mul(mul(sf, qk), k14);
        out.push_back(fq);
        out.push_back(mul(st, fr30_const_one270()));
        // k_lk_constraints
        const Fr30 F = add(kF, beta, fq);
        const Fr30 Tt = add(kTt, beta, st);
        const Fr30 D = add(kD, phir, phi, -1);
        const Fr30 E = add(kE, m, mul(mul(D, Tt), k14));
        Fr30 W = add(kW, mul(mul(E, F), k14), Tt, -1);
        W = add(kW, W, mul(mul(l0, phi), ak14));
        out.push_back(mul(W, a3));
    }
    for (int i = 0; i < kReports; i++) printf("%llu%c", (unsigned long long)rep[i], i + 1 < kReports ? ' ' : '\n');
    for (const Fr30& v : out) print(v);
    return 0;
}
