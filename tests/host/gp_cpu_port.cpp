// CPU comparison for tests/perf_grand_product.py: the same z_0 = 1, z_(i+1) = z_i A_i / B_i over csrc/host_fr.hpp (a 4 x u64
// Montgomery field, plain C++), with Montgomery's trick -- one inversion per thread's chunk.  A PORT of the device algorithm to
// the host for scale, like tools' cpu_baseline: not a tuned CPU library.  Stand-alone: g++ -O2 -pthread.
//
// usage: gp_cpu_port log_n t threads reps   -> one line per repetition: seconds; then a checksum (z_n, hex) on the last line
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <chrono>
#include <thread>
#include <vector>

#include "../../kzg_poly_commit_exploration_amd/csrc/host_fr.hpp"

using kzg_host::Fr;
using kzg_host::fr_mul;

int main(int argc, char** argv) {
    if (argc != 5) return 2;
    const size_t n = (size_t)1 << atoi(argv[1]);
    const int t = atoi(argv[2]), threads = atoi(argv[3]), reps = atoi(argv[4]);
    if (t < 1 || t > 16 || threads < 1 || threads > 64 || reps < 1 || n % (size_t)threads) return 2;
    // 2 t columns of non-zero values: powers of a fixed element
    std::vector<Fr> cols(2 * (size_t)t * n);
    Fr g = kzg_host::fr_add(kzg_host::kFrOne, kzg_host::kFrOne), v = g;
    g = kzg_host::fr_add(g, kzg_host::kFrOne);
    for (Fr& c : cols) {
        c = v;
        v = fr_mul(v, g);
    }
    std::vector<Fr> z(n), pa(n), pb(n);
    const size_t chunk = n / (size_t)threads;
    std::vector<Fr> ratio(threads);
    Fr last = kzg_host::kFrOne;
    for (int r = 0; r < reps; r++) {
        const auto t0 = std::chrono::steady_clock::now();
        auto local = [&](int w) {  // z of the chunk as if it began at one; ratio[w] = prod A / prod B of the chunk
            const size_t lo = (size_t)w * chunk, hi = lo + chunk;
            Fr a = kzg_host::kFrOne, b = kzg_host::kFrOne;
            for (size_t i = lo; i < hi; i++) {  // exclusive prefix of A, inclusive prefix of B
                pa[i] = a;
                Fr ai = cols[i], bi = cols[(size_t)t * n + i];
                for (int j = 1; j < t; j++) {
                    ai = fr_mul(ai, cols[(size_t)j * n + i]);
                    bi = fr_mul(bi, cols[(size_t)(t + j) * n + i]);
                }
                a = fr_mul(a, ai);
                b = fr_mul(b, bi);
                z[i] = bi;  // kept for the way back
                pb[i] = b;
            }
            Fr inv = kzg_host::fr_inv(b);  // 1 / (B_lo .. B_(hi-1))
            ratio[w] = fr_mul(a, inv);
            for (size_t i = hi; i-- > lo;) {  // inv = 1 / (B_lo .. B_i); z_i needs 1 / (B_lo .. B_(i-1))
                inv = fr_mul(inv, z[i]);
                z[i] = fr_mul(pa[i], inv);
            }
        };
        auto scale = [&](int w, Fr c) {
            for (size_t i = (size_t)w * chunk; i < (size_t)(w + 1) * chunk; i++) z[i] = fr_mul(z[i], c);
        };
        std::vector<std::thread> pool;
        for (int w = 1; w < threads; w++) pool.emplace_back(local, w);
        local(0);
        for (auto& th : pool) th.join();
        pool.clear();
        Fr c = ratio[0];
        for (int w = 1; w < threads; w++) {
            pool.emplace_back(scale, w, c);
            c = fr_mul(c, ratio[w]);
        }
        for (auto& th : pool) th.join();
        last = c;
        printf("%.6f\n", std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
    }
    printf("%016llx%016llx%016llx%016llx\n", (unsigned long long)last.l[3], (unsigned long long)last.l[2], (unsigned long long)last.l[1],
           (unsigned long long)last.l[0]);
    return z[n - 1].l[0] == 0 && z[n - 1].l[1] == 0 && z[n - 1].l[2] == 0 && z[n - 1].l[3] == 0;
}
