// CPU comparison for tests/perf_lookup.py: the route a caller takes without the device calls, over csrc/host_fr.hpp (a 4 x u64
// Montgomery field, plain C++).  A PORT for scale, like gp_cpu_port.cpp: not a tuned CPU library.  Stand-alone: g++ -O2 -pthread.
//
// usage: lu_cpu_port sum  log_n k threads reps     the lookup form's running sum: per row the k + 1 fractions as one pair (N, D),
//                                                  Montgomery's trick over each thread's chunk (one inversion per chunk), the
//                                                  chunk's running sum, then the chunk offsets
//        lu_cpu_port mult log_n k threads reps d   the multiplicities by a std::unordered_map from the 32 bytes of a value to its
//                                                  least row (built by one thread), the k n lookups counted by `threads` threads;
//                                                  d = 0: uniform lookups, 1: every lookup on one row, 2: a table whose images are
//                                                  0, 1, 2, ..
// -> one line per repetition: seconds; then a checksum on the last line
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <atomic>
#include <chrono>
#include <thread>
#include <unordered_map>
#include <vector>

#include "../../kzg_poly_commit_exploration_amd/csrc/host_fr.hpp"

using kzg_host::Fr;
using kzg_host::fr_add;
using kzg_host::fr_mul;
using kzg_host::fr_sub;

namespace {
struct Key {
    uint64_t l[4];
    bool operator==(const Key& o) const { return memcmp(l, o.l, 32) == 0; }
};
struct KeyHash {
    size_t operator()(const Key& k) const {
        uint64_t h = 0x9e3779b97f4a7c15ULL;
        for (int i = 0; i < 4; i++) {
            h ^= k.l[i];
            h *= 0xff51afd7ed558ccdULL;
            h ^= h >> 33;
        }
        return (size_t)h;
    }
};
double now() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

int run_sum(size_t n, int k, int threads, int reps) {
    if (n % (size_t)threads) return 2;
    std::vector<Fr> cols((size_t)(k + 2) * n);  // k lookup columns, the table, the multiplicities: powers of a fixed element
    Fr g = fr_add(kzg_host::kFrOne, kzg_host::kFrOne), v = g;
    g = fr_add(g, kzg_host::kFrOne);
    for (Fr& c : cols) {
        c = v;
        v = fr_mul(v, g);
    }
    const Fr beta = v, zero = fr_sub(v, v);
    std::vector<Fr> phi(n), num(n), pre(n);
    const size_t chunk = n / (size_t)threads;
    std::vector<Fr> total(threads);
    Fr last = zero;
    for (int r = 0; r < reps; r++) {
        const double t0 = now();
        auto local = [&](int w) {
            const size_t lo = (size_t)w * chunk, hi = lo + chunk;
            Fr run = kzg_host::kFrOne;
            for (size_t i = lo; i < hi; i++) {
                Fr d = fr_add(cols[i], beta), nn = kzg_host::kFrOne;
                for (int j = 1; j < k; j++) {
                    const Fr b = fr_add(cols[(size_t)j * n + i], beta);
                    nn = fr_add(fr_mul(nn, b), d);
                    d = fr_mul(d, b);
                }
                const Fr b = fr_add(cols[(size_t)k * n + i], beta);
                nn = fr_sub(fr_mul(nn, b), fr_mul(cols[(size_t)(k + 1) * n + i], d));
                d = fr_mul(d, b);
                num[i] = nn;
                phi[i] = d;  // kept for the way back
                pre[i] = run;
                run = fr_mul(run, d);
            }
            Fr inv = kzg_host::fr_inv(run);
            for (size_t i = hi; i-- > lo;) {  // h_i = N_i / D_i
                const Fr h = fr_mul(num[i], fr_mul(pre[i], inv));
                inv = fr_mul(inv, phi[i]);
                num[i] = h;
            }
            Fr acc = zero;
            for (size_t i = lo; i < hi; i++) {
                phi[i] = acc;
                acc = fr_add(acc, num[i]);
            }
            total[w] = acc;
        };
        auto shift = [&](int w, Fr c) {
            for (size_t i = (size_t)w * chunk; i < (size_t)(w + 1) * chunk; i++) phi[i] = fr_add(phi[i], c);
        };
        std::vector<std::thread> pool;
        for (int w = 1; w < threads; w++) pool.emplace_back(local, w);
        local(0);
        for (auto& th : pool) th.join();
        pool.clear();
        Fr c = total[0];
        for (int w = 1; w < threads; w++) {
            pool.emplace_back(shift, w, c);
            c = fr_add(c, total[w]);
        }
        for (auto& th : pool) th.join();
        last = c;
        printf("%.6f\n", now() - t0);
    }
    printf("%016llx%016llx\n", (unsigned long long)last.l[3], (unsigned long long)phi[n - 1].l[0]);
    return 0;
}

int run_mult(size_t n, int k, int threads, int reps, int dist) {
    std::vector<Key> table(n), looks((size_t)k * n);
    uint64_t s = 0x243f6a8885a308d3ULL;
    auto rnd = [&]() {
        s ^= s << 13;
        s ^= s >> 7;
        s ^= s << 17;
        return s;
    };
    for (size_t i = 0; i < n; i++) {
        if (dist == 2) table[i] = Key{{(uint64_t)i, 0, 0, 0}};
        else table[i] = Key{{rnd(), rnd(), rnd(), rnd() >> 2}};
    }
    for (Key& q : looks) q = table[dist == 1 ? 77 % n : rnd() % n];
    Fr r2 = kzg_host::kFrOne;  // 2^512: takes a plain count to its image
    for (int i = 0; i < 256; i++) r2 = fr_add(r2, r2);
    uint64_t sum = 0;
    for (int r = 0; r < reps; r++) {
        const double t0 = now();
        std::unordered_map<Key, uint32_t, KeyHash> least;
        least.reserve(2 * n);
        for (size_t i = 0; i < n; i++) least.emplace(table[i], (uint32_t)i);  // the first row stays
        std::vector<std::atomic<uint32_t>> counts(n);
        for (auto& c : counts) c.store(0, std::memory_order_relaxed);
        std::atomic<uint64_t> missing{0};
        auto probe = [&](int w) {
            const size_t per = (looks.size() + threads - 1) / threads, lo = (size_t)w * per;
            const size_t hi = lo + per < looks.size() ? lo + per : looks.size();
            for (size_t i = lo; i < hi; i++) {
                const auto it = least.find(looks[i]);
                if (it == least.end()) missing.fetch_add(1);
                else counts[it->second].fetch_add(1, std::memory_order_relaxed);
            }
        };
        std::vector<std::thread> pool;
        for (int w = 1; w < threads; w++) pool.emplace_back(probe, w);
        probe(0);
        for (auto& th : pool) th.join();
        std::vector<Fr> mult(n);  // the counts as images
        for (size_t i = 0; i < n; i++) {
            Fr c{};
            c.l[0] = counts[i].load(std::memory_order_relaxed);
            mult[i] = fr_mul(c, r2);
        }
        printf("%.6f\n", now() - t0);
        sum += mult[dist == 1 ? 77 % n : 0].l[0] + missing.load();
    }
    printf("%016llx\n", (unsigned long long)sum);
    return 0;
}
}  // namespace

int main(int argc, char** argv) {
    if (argc < 6) return 2;
    const size_t n = (size_t)1 << atoi(argv[2]);
    const int k = atoi(argv[3]), threads = atoi(argv[4]), reps = atoi(argv[5]);
    if (k < 1 || k > 15 || threads < 1 || threads > 16 || reps < 1) return 2;
    if (!strcmp(argv[1], "sum")) return run_sum(n, k, threads, reps);
    if (!strcmp(argv[1], "mult") && argc == 7) return run_mult(n, k, threads, reps, atoi(argv[6]));
    return 2;
}
