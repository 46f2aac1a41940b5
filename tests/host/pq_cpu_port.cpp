// CPU comparison for tests/perf_perm_quotient.py: the pointwise work of the permutation quotient that a caller without
// kzg_permutation_quotient has to do on the host between the transforms -- the twist of the coefficients by g^i, Num(x_i) / Z_H(x_i)
// at the N = e n coset points, the untwist of the quotient -- over csrc/host_fr.hpp (a 4 x u64 Montgomery field, plain C++).  A PORT
// for scale, like gp_cpu_port.cpp: not a tuned CPU library.  Stand-alone: g++ -O2 -pthread.
//
// usage: pq_cpu_port log_n log_ext t threads reps   -> one line per repetition: seconds of the twist of 2 t + 1 columns, of the
//                                                      constraints, of the untwist; then a checksum on the last line
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <chrono>
#include <functional>
#include <thread>
#include <vector>

#include "../../kzg_poly_commit_exploration_amd/csrc/host_fr.hpp"

using kzg_host::Fr;
using kzg_host::fr_add;
using kzg_host::fr_mul;
using kzg_host::fr_sub;

static void parallel(int threads, size_t count, const std::function<void(size_t, size_t)>& body) {
    const size_t chunk = count / (size_t)threads;
    std::vector<std::thread> pool;
    for (int w = 1; w < threads; w++) pool.emplace_back(body, (size_t)w * chunk, (size_t)(w + 1) * chunk);
    body(0, chunk);
    for (auto& th : pool) th.join();
}

int main(int argc, char** argv) {
    if (argc != 6) return 2;
    const int log_n = atoi(argv[1]), log_ext = atoi(argv[2]), t = atoi(argv[3]), threads = atoi(argv[4]), reps = atoi(argv[5]);
    if (log_n < 4 || log_n + log_ext > 22 || log_ext < 1 || log_ext > 3 || t < 1 || t > 7 || threads < 1 || threads > 64 || reps < 1) return 2;
    const size_t n = (size_t)1 << log_n, e = (size_t)1 << log_ext, N = n * e;
    if (n % (size_t)threads) return 2;
    Fr g = kzg_host::kFrOne;
    for (int i = 0; i < 6; i++) g = fr_add(g, kzg_host::kFrOne);
    const Fr w = kzg_host::fr_domain_root((unsigned)(log_n + log_ext));
    // 2 t + 1 coefficient columns of n values and, as stand-ins for the transforms' outputs, 2 t + 3 columns of N values
    const size_t ncols = 2 * (size_t)t + 1;
    std::vector<Fr> coef(ncols * n), ext((ncols + 2) * N), out(N);
    Fr v = fr_add(g, g);
    for (Fr& c : coef) c = v, v = fr_mul(v, g);
    for (Fr& c : ext) c = v, v = fr_mul(v, g);
    Fr shifts[8], zinv[8];
    for (int j = 0; j < 8; j++) shifts[j] = kzg_host::fr_pow(g, (uint64_t)j), zinv[j] = kzg_host::fr_pow(g, (uint64_t)(j + 11));
    const Fr alpha = kzg_host::fr_pow(g, 1001), beta = kzg_host::fr_pow(g, 1003), gamma = kzg_host::fr_pow(g, 1007);
    const Fr alpha2 = fr_mul(alpha, alpha), ginv = kzg_host::fr_inv(g);
    for (int r = 0; r < reps; r++) {
        auto t0 = std::chrono::steady_clock::now();
        parallel(threads, n, [&](size_t lo, size_t hi) {  // c_i g^i for every column
            Fr p = kzg_host::fr_pow(g, lo);
            for (size_t i = lo; i < hi; i++, p = fr_mul(p, g))
                for (size_t c = 0; c < ncols; c++) coef[c * n + i] = fr_mul(coef[c * n + i], p);
        });
        auto t1 = std::chrono::steady_clock::now();
        parallel(threads, N, [&](size_t lo, size_t hi) {
            const Fr *f = ext.data(), *s = f + (size_t)t * N, *z = s + (size_t)t * N, *l0 = z + N, *gate = l0 + N;
            Fr x = fr_mul(g, kzg_host::fr_pow(w, lo));
            for (size_t i = lo; i < hi; i++, x = fr_mul(x, w)) {
                Fr a = z[i], b = z[(i + e) & (N - 1)];
                for (int j = 0; j < t; j++) {
                    const Fr fg = fr_add(f[(size_t)j * N + i], gamma);
                    a = fr_mul(a, fr_add(fg, fr_mul(fr_mul(beta, shifts[j]), x)));
                    b = fr_mul(b, fr_add(fg, fr_mul(beta, s[(size_t)j * N + i])));
                }
                Fr num = fr_add(gate[i], fr_mul(alpha, fr_sub(a, b)));
                num = fr_add(num, fr_mul(alpha2, fr_mul(fr_sub(z[i], kzg_host::kFrOne), l0[i])));
                out[i] = fr_mul(num, zinv[i & (e - 1)]);
            }
        });
        auto t2 = std::chrono::steady_clock::now();
        parallel(threads, N, [&](size_t lo, size_t hi) {  // q_i g^-i
            Fr p = kzg_host::fr_pow(ginv, lo);
            for (size_t i = lo; i < hi; i++, p = fr_mul(p, ginv)) out[i] = fr_mul(out[i], p);
        });
        auto t3 = std::chrono::steady_clock::now();
        printf("%.6f %.6f %.6f\n", std::chrono::duration<double>(t1 - t0).count(), std::chrono::duration<double>(t2 - t1).count(),
               std::chrono::duration<double>(t3 - t2).count());
    }
    printf("%016llx\n", (unsigned long long)(out[N - 1].l[0] ^ coef[n - 1].l[3]));
    return 0;
}
