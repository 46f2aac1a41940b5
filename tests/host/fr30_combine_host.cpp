// Host build of the accumulate step of the combined openings (csrc/fr30.hip.h: fr30_mac, fr30_sum_reduce) for
// tests/test_open_combined.py (plain g++; the header is __host__ __device__ code).  Test infrastructure only.
#include <stdint.h>
#include <string.h>

#include "../../kzg_poly_commit_exploration_amd/csrc/fr30.hip.h"
#include "../../kzg_poly_commit_exploration_amd/csrc/host_fr.hpp"
#include "../../kzg_poly_commit_exploration_amd/csrc/fr30_host.hpp"

using namespace kzg;

namespace {
int64_t mag(int32_t v) { return v < 0 ? -(int64_t)v : (int64_t)v; }
}  // namespace

extern "C" {

// the bounds the comment above fr30_mac claims: raw digits 0..7, normalised digits 0..7, the top digit
void r30c_bounds(int64_t out[3]) {
    out[0] = kR9SumRawBound;
    out[1] = kR9SumNormBound;
    out[2] = kR9SumTopBound;
}

// acc = start (8 x u32, a canonical value or zero, loaded as the kernel loads F); then `count` times acc = fr30_mac(acc,
// coefficient k (8 x u32 at coeffs + 8 k), multiplier k (blst_fr image of w, 4 x u64 at mults + 4 k, prepared as the host
// prepares gamma^i)).  acc_out: the digits before the reduction; limbs_out: fr30_to_limbs(fr30_sum_reduce(acc)).
// maxima[0..2]: the largest |digit 0..7| of any raw sum, of any normalised sum (the start included), and |digit 8| seen.
void r30c_sum(const uint32_t* start, const uint32_t* coeffs, const uint64_t* mults, int count, int32_t* acc_out,
              uint32_t* limbs_out, int64_t maxima[3]) {
    maxima[0] = maxima[1] = maxima[2] = 0;
    auto see = [&](const Fr30& v, int which) {
        for (int i = 0; i < kR9 - 1; i++)
            if (mag(v.d[i]) > maxima[which]) maxima[which] = mag(v.d[i]);
        if (mag(v.d[kR9 - 1]) > maxima[2]) maxima[2] = mag(v.d[kR9 - 1]);
    };
    Fr30 acc = fr30_from_limbs(start);
    see(acc, 1);
    for (int k = 0; k < count; k++) {
        const Fr30 c = fr30_from_limbs(coeffs + 8 * k);
        kzg_host::Fr w;
        memcpy(w.l, mults + 4 * k, 32);
        const Fr30 g = fr30_arg_from_mont256(w);
        const Fr30 raw = fr30_mac_raw(acc, c, g);
        see(raw, 0);
        acc = fr30_mac(acc, c, g);
        see(acc, 1);
        const Fr30 again = fr30_norm(raw);  // fr30_mac is the carry pass over fr30_mac_raw
        if (memcmp(again.d, acc.d, sizeof acc.d) != 0) maxima[0] = INT64_MAX;
    }
    memcpy(acc_out, acc.d, sizeof acc.d);
    fr30_to_limbs(fr30_sum_reduce(acc), limbs_out);
}

}  // extern "C"
