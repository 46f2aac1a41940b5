// Host build of fr30_inv (csrc/fr30.hip.h) for tests/test_verify_openings.py (plain g++; the header is __host__ __device__
// code).  Test infrastructure only.
#include <stdint.h>
#include <string.h>

#include "../../kzg_poly_commit_exploration_amd/csrc/fr30.hip.h"

using namespace kzg;

extern "C" {

void r30_inv(const int32_t* a, int32_t* r) {
    Fr30 x;
    memcpy(x.d, a, sizeof x.d);
    Fr30 z = fr30_inv(x);
    memcpy(r, z.d, sizeof z.d);
}
void r30_mul(const int32_t* a, const int32_t* b, int32_t* r) {
    Fr30 x, y;
    memcpy(x.d, a, sizeof x.d);
    memcpy(y.d, b, sizeof y.d);
    Fr30 z = fr30_mul(x, y);
    memcpy(r, z.d, sizeof z.d);
}
}
