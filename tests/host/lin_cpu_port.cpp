// CPU comparison for tests/perf_circuit_open.py: the host work of the last round that a caller without kzg_circuit_open has to do
// between downloading the key's coefficients and calling kzg_open_sets -- the 2 t evaluations at zeta (Horner per thread chunk, the
// chunks joined by powers of zeta) and r[i] = sum_k scalar_k C_k[i] over the t + e + 3 columns -- over csrc/host_fr.hpp (a 4 x u64
// Montgomery field, plain C++).  A PORT for scale, like pq_cpu_port.cpp: not a tuned CPU library.  Stand-alone: g++ -O2 -pthread.
//
// usage: lin_cpu_port log_n log_ext t threads reps   -> one line per repetition: seconds of the evaluations, of r; then a checksum
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

static void parallel(int threads, size_t count, const std::function<void(int, size_t, size_t)>& body) {
    const size_t chunk = count / (size_t)threads;
    std::vector<std::thread> pool;
    for (int w = 1; w < threads; w++) pool.emplace_back(body, w, (size_t)w * chunk, (size_t)(w + 1) * chunk);
    body(0, 0, chunk);
    for (auto& th : pool) th.join();
}

int main(int argc, char** argv) {
    if (argc != 6) return 2;
    const int log_n = atoi(argv[1]), log_ext = atoi(argv[2]), t = atoi(argv[3]), threads = atoi(argv[4]), reps = atoi(argv[5]);
    if (log_n < 4 || log_n + log_ext > 22 || log_ext < 1 || log_ext > 3 || t < 2 || t > 7 || threads < 1 || threads > 64 || reps < 1) return 2;
    const size_t n = (size_t)1 << log_n, e = (size_t)1 << log_ext;
    if (n % (size_t)threads) return 2;
    Fr g = kzg_host::kFrOne;
    for (int i = 0; i < 6; i++) g = fr_add(g, kzg_host::kFrOne);
    const size_t nev = 2 * (size_t)t, ncols = (size_t)t + e + 3;
    std::vector<Fr> ev_cols(nev * n), cols(ncols * n), r(n), scal(ncols), part(nev * (size_t)threads), ys(nev);
    Fr v = fr_add(g, g);
    for (Fr& c : ev_cols) c = v, v = fr_mul(v, g);
    for (Fr& c : cols) c = v, v = fr_mul(v, g);
    for (Fr& c : scal) c = v, v = fr_mul(v, g);
    const Fr zeta = kzg_host::fr_pow(g, 1009);
    for (int rep = 0; rep < reps; rep++) {
        auto t0 = std::chrono::steady_clock::now();
        parallel(threads, n, [&](int w, size_t lo, size_t hi) {  // sum_{lo <= i < hi} c_i zeta^(i - lo)
            for (size_t c = 0; c < nev; c++) {
                Fr h = ev_cols[c * n + hi - 1];
                for (size_t i = hi - 1; i-- > lo;) h = fr_add(fr_mul(h, zeta), ev_cols[c * n + i]);
                part[c * (size_t)threads + (size_t)w] = h;
            }
        });
        const Fr step = kzg_host::fr_pow(zeta, n / (size_t)threads);
        for (size_t c = 0; c < nev; c++) {
            Fr h = part[c * (size_t)threads + (size_t)threads - 1];
            for (int w = threads - 1; w-- > 0;) h = fr_add(fr_mul(h, step), part[c * (size_t)threads + (size_t)w]);
            ys[c] = h;
        }
        auto t1 = std::chrono::steady_clock::now();
        parallel(threads, n, [&](int, size_t lo, size_t hi) {
            for (size_t i = lo; i < hi; i++) {
                Fr acc = fr_mul(scal[0], cols[i]);
                for (size_t k = 1; k < ncols; k++) acc = fr_add(acc, fr_mul(scal[k], cols[k * n + i]));
                r[i] = acc;
            }
        });
        auto t2 = std::chrono::steady_clock::now();
        printf("%.6f %.6f\n", std::chrono::duration<double>(t1 - t0).count(), std::chrono::duration<double>(t2 - t1).count());
    }
    printf("%016llx\n", (unsigned long long)(r[n - 1].l[0] ^ ys[nev - 1].l[3]));
    return 0;
}
