// Host build of csrc/msm_recode.h for tests/test_msm_recode_host.py (plain g++; the header is __host__ __device__ code).
// Test infrastructure only.
#include <stdint.h>
#include <string.h>

#include "../../kzg_poly_commit_exploration_amd/csrc/msm_recode.h"

using namespace kzg;

namespace {
// (level, bucket, negative) triples, at most cap of them; n counts every digit the loop reports
struct Sink {
    uint32_t* out;
    int cap, n;
    void operator()(uint32_t level, uint32_t bucket, bool neg) {
        if (n < cap) {
            out[3 * n] = level;
            out[3 * n + 1] = bucket;
            out[3 * n + 2] = neg ? 1u : 0u;
        }
        n++;
    }
};
template <uint32_t C>
void fixed(const uint32_t* k, Sink& s) {
    for_each_window_digit_fixed<C>(k, s);
}
}  // namespace

extern "C" {

// the fold: image (blst_fr image when is_mont, canonical limbs otherwise) -> |k| in k[8]; returns the negate flag
int recode_host_fold(const uint32_t* image, int is_mont, uint32_t* k) { return recode_fold(image, is_mont, k) ? 1 : 0; }

// the 32-byte record: pack (k, flip) into rec, unpack it again into k_out; returns the flag that came back
int recode_host_pack_roundtrip(const uint32_t* k, int flip, uint32_t* rec, uint32_t* k_out) {
    memcpy(rec, k, 32);
    recode_pack(rec, flip != 0);
    memcpy(k_out, rec, 32);
    return recode_unpack(k_out) ? 1 : 0;
}

// the window digits of k at width c through the run-time loop: returns their number
int recode_host_windows_runtime(const uint32_t* k, uint32_t c, uint32_t* out, int cap) {
    uint32_t t[8];
    memcpy(t, k, 32);
    Sink s{out, cap, 0};
    for_each_window_digit(t, c, (255 + c - 1) / c, s);
    return s.n;
}

// ... through the form compiled for the width (8 <= c <= 20); -1 for another width
int recode_host_windows_fixed(const uint32_t* k, uint32_t c, uint32_t* out, int cap) {
    Sink s{out, cap, 0};
    switch (c) {
        case 8: fixed<8>(k, s); break;
        case 9: fixed<9>(k, s); break;
        case 10: fixed<10>(k, s); break;
        case 11: fixed<11>(k, s); break;
        case 12: fixed<12>(k, s); break;
        case 13: fixed<13>(k, s); break;
        case 14: fixed<14>(k, s); break;
        case 15: fixed<15>(k, s); break;
        case 16: fixed<16>(k, s); break;
        case 17: fixed<17>(k, s); break;
        case 18: fixed<18>(k, s); break;
        case 19: fixed<19>(k, s); break;
        case 20: fixed<20>(k, s); break;
        default: return -1;
    }
    return s.n;
}

// the width-c non-adjacent form of k: (bit position, bucket, negative)
int recode_host_naf(const uint32_t* k, uint32_t c, uint32_t* out, int cap) {
    Sink s{out, cap, 0};
    for_each_naf_digit(k, c, s);
    return s.n;
}
}
