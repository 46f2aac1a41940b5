// The folds of a multilinear opening on the host (csrc/host_fr.hpp arithmetic, `threads` threads per level), for
// tests/perf_multilinear.py: the route a caller had before kzg_ml_fold.  Measurement infrastructure only; built with g++ -O2
// -shared -pthread by the script.
#include <stdint.h>

#include <cstring>
#include <thread>
#include <vector>

#include "../../kzg_poly_commit_exploration_amd/csrc/host_fr.hpp"

using kzg_host::Fr;

// pyr: the n - 1 values of f_1 .. f_ell, level i at offset n - (n >> (i - 1)); all blst_fr images
extern "C" void ml_fold_cpu(const uint64_t* evals, unsigned ell, const uint64_t* us, uint64_t* pyr, int threads) {
    const size_t n = (size_t)1 << ell;
    const Fr* src = reinterpret_cast<const Fr*>(evals);
    Fr* dst = reinterpret_cast<Fr*>(pyr);
    for (unsigned i = 0; i < ell; i++) {
        const size_t len = n >> (i + 1);
        Fr u;
        std::memcpy(u.l, us + 4 * i, 32);
        auto work = [&](size_t lo, size_t hi) {
            for (size_t j = lo; j < hi; j++)
                dst[j] = kzg_host::fr_add(src[2 * j], kzg_host::fr_mul(u, kzg_host::fr_sub(src[2 * j + 1], src[2 * j])));
        };
        const size_t T = len >= 4096 && threads > 1 ? (size_t)threads : 1;
        if (T == 1) {
            work(0, len);
        } else {
            std::vector<std::thread> pool;
            for (size_t t = 0; t < T; t++) pool.emplace_back(work, len * t / T, len * (t + 1) / T);
            for (auto& th : pool) th.join();
        }
        src = dst;
        dst += len;
    }
}
