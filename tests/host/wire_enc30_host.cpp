// Host build of csrc/wire_enc30.hip.h for tests/test_blob_bytes.py (plain g++; the header is __host__ __device__ code).
// Test infrastructure only: the two encoders and, for the round trips, wire30.hip.h's decoders over a C ABI.
#include <stdint.h>
#include <string.h>

#include "../../kzg_poly_commit_exploration_amd/csrc/wire_enc30.hip.h"

using namespace kzg;

extern "C" {

// x and y as 13 signed digits each (Montgomery 2^390; all zero = infinity) -> 48 bytes
void we30_g1_encode(const int32_t* x, const int32_t* y, uint8_t* out48) {
    Fq fx, fy;
    memcpy(fx.d, x, sizeof fx.d);
    memcpy(fy.d, y, sizeof fy.d);
    uint32_t raw[12];
    wire_g1_encode(fx, fy, raw);
    memcpy(out48, raw, 48);
}

// the blst_fr image as 8 x u32 -> status (kWireBad when not below r), 32 big-endian bytes
uint32_t we30_fr_encode(const uint32_t* in, uint8_t* out32) {
    uint32_t raw[8];
    const uint32_t st = wire_fr_encode(in, raw);
    memcpy(out32, raw, 32);
    return st;
}

uint32_t we30_g1_decode(const uint8_t* in48, int32_t* x, int32_t* y) {
    uint32_t raw[12];
    memcpy(raw, in48, 48);
    Fq fx, fy;
    const uint32_t st = wire_g1_decode(raw, fx, fy);
    memcpy(x, fx.d, sizeof fx.d);
    memcpy(y, fy.d, sizeof fy.d);
    return st;
}

uint32_t we30_fr_decode(const uint8_t* in32, uint32_t* out) {
    uint32_t raw[8];
    memcpy(raw, in32, 32);
    return wire_fr_decode(raw, out);
}
}
