// Host build of csrc/wire30.hip.h for tests/test_wire_bytes.py (plain g++; the header is __host__ __device__ code).
// Test infrastructure only: the two decoders over a C ABI, on the bytes as they travel.
#include <stdint.h>
#include <string.h>

#include "../../kzg_poly_commit_exploration_amd/csrc/wire30.hip.h"

using namespace kzg;

extern "C" {

// 48 bytes -> status (kWireInfinity | kWireBad), x and y as 13 signed digits each (Montgomery 2^390, lazily reduced)
uint32_t w30_g1_decode(const uint8_t* in48, int32_t* x, int32_t* y) {
    uint32_t raw[12];
    memcpy(raw, in48, 48);
    Fq fx, fy;
    const uint32_t st = wire_g1_decode(raw, fx, fy);
    memcpy(x, fx.d, sizeof fx.d);
    memcpy(y, fy.d, sizeof fy.d);
    return st;
}

// 32 big-endian bytes -> status (kWireBad when not below r), the blst_fr image as 8 x u32
uint32_t w30_fr_decode(const uint8_t* in32, uint32_t* out) {
    uint32_t raw[8];
    memcpy(raw, in32, 32);
    return wire_fr_decode(raw, out);
}

uint32_t w30_brp(uint32_t i, uint32_t bits) { return wire_brp(i, bits); }
}
