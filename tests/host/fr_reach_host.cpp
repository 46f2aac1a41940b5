// Host replay of the Fr kernels' accumulation patterns on the unchanged csrc/fr30.hip.h, for tests/test_fr_extremes.py
// (plain g++ -fwrapv; the header is __host__ __device__ code).  Test infrastructure only.
//
// Each function replays ONE pattern -- the order of products, raw sums, carry passes and reductions of a kernel, not its
// memory layout -- on inputs given as blst_fr images (8 x u32) and multipliers given as blst_fr images of w (4 x u64,
// prepared with fr30_arg_from_mont256 as the host prepares them), returns the canonical result and reports
//     rep[0]  the largest |digit 0..7| that enters a carry pass or a product as a raw sum
//     rep[1]  the largest |digit 0..7| that leaves a carry pass
//     rep[2]  the largest |digit 8|
//     rep[3]  the largest |column| of any product, in exact (__int128) arithmetic, saturated at 2^64 - 1
// Raw sums are formed in 64 bits and then wrapped to 32 as the device would, so a weakened variant that overflows shows
// both in the report and in a wrong result.
#include <stdint.h>
#include <string.h>

#include <vector>

#include "../../kzg_poly_commit_exploration_amd/csrc/fr30.hip.h"
#include "../../kzg_poly_commit_exploration_amd/csrc/host_fr.hpp"
#include "../../kzg_poly_commit_exploration_amd/csrc/fr30_host.hpp"

using namespace kzg;

namespace {

struct Rep {
    uint64_t* r;
    void digits(const Fr30& v, int which) {
        for (int i = 0; i < kR9 - 1; i++) see(which, v.d[i]);
        see(2, v.d[kR9 - 1]);
    }
    void see(int which, int64_t v) {
        const uint64_t m = v < 0 ? (uint64_t)(-v) : (uint64_t)v;
        if (m > r[which]) r[which] = m;
    }
    void column(__int128 acc) {
        const __int128 m = acc < 0 ? -acc : acc;
        const uint64_t s = m > (__int128)UINT64_MAX ? UINT64_MAX : (uint64_t)m;
        if (s > r[3]) r[3] = s;
    }
};

// fr30_mul with its columns followed in exact arithmetic (the Montgomery digits depend on the low 30 bits only, so they are
// the ones the 64-bit accumulator makes whether it overflows or not); the product itself is the header's
Fr30 mul(Rep& rep, const Fr30& a, const Fr30& b) {
    int32_t m[kR9];
    __int128 acc = 0;
    for (int k = 0; k < kR9; k++) {
        for (int i = 0; i <= k; i++) acc += (__int128)a.d[i] * b.d[k - i];
        for (int j = 0; j < k; j++) acc += (__int128)m[j] * fr30_rd(k - j);
        rep.column(acc);
        m[k] = fr30_sext30(0u - (uint32_t)(uint64_t)acc);
        acc += m[k];
        acc >>= kR9Bits;
    }
    for (int k = kR9; k < 2 * kR9 - 1; k++) {
        for (int i = k - kR9 + 1; i < kR9; i++) acc += (__int128)a.d[i] * b.d[k - i];
        for (int j = k - kR9 + 1; j < kR9; j++) acc += (__int128)m[j] * fr30_rd(k - j);
        rep.column(acc);
        acc = (acc + (1 << (kR9Bits - 1))) >> kR9Bits;
    }
    const Fr30 p = fr30_mul(a, b);
    rep.digits(p, 1);  // a product's digits 0..7 are in [-2^29, 2^29)
    return p;
}
// a + sign b digit-wise: reported in 64 bits, wrapped to 32
Fr30 add_raw(Rep& rep, const Fr30& a, const Fr30& b, int sign = 1) {
    Fr30 r;
    for (int i = 0; i < kR9; i++) {
        const int64_t s = (int64_t)a.d[i] + sign * (int64_t)b.d[i];
        rep.see(i < kR9 - 1 ? 0 : 2, s);
        r.d[i] = (int32_t)(uint32_t)(uint64_t)s;
    }
    return r;
}
Fr30 norm(Rep& rep, const Fr30& a) {
    const Fr30 r = fr30_norm(a);
    rep.digits(r, 1);
    return r;
}
Fr30 add(Rep& rep, const Fr30& a, const Fr30& b) { return norm(rep, add_raw(rep, a, b)); }
Fr30 sub(Rep& rep, const Fr30& a, const Fr30& b) { return norm(rep, add_raw(rep, a, b, -1)); }
Fr30 load(Rep& rep, const uint32_t* l) {
    const Fr30 v = fr30_from_limbs(l);
    rep.digits(v, 1);
    return v;
}
Fr30 mult(const uint64_t* image) {
    kzg_host::Fr w;
    memcpy(w.l, image, 32);
    return fr30_arg_from_mont256(w);
}
Rep start(uint64_t* rep) {
    rep[0] = rep[1] = rep[2] = rep[3] = 0;
    return Rep{rep};
}

}  // namespace

extern "C" {

void fre_bounds(int64_t out[3]) {
    out[0] = kR9SumRawBound;
    out[1] = kR9SumNormBound;
    out[2] = kR9SumTopBound;
}

// k_combine_eval's accumulator: acc = start, then `count` times acc = fr30_mac(acc, coefficient k, multiplier k); out =
// fr30_to_limbs(fr30_sum_reduce(acc)).  every = 1 is the kernel.  every = 2 is the WEAKENED variant (a carry pass after every
// second product only; never on a device).
void fre_mac(const uint32_t* start_image, const uint32_t* coeffs, const uint64_t* mults, int count, int every, uint32_t* out,
             uint64_t* report) {
    Rep rep = start(report);
    Fr30 acc = load(rep, start_image);
    for (int k = 0; k < count; k++) {
        acc = add_raw(rep, acc, mul(rep, load(rep, coeffs + 8 * k), mult(mults + 4 * k)));
        if ((k + 1) % every == 0 || k + 1 == count) acc = norm(rep, acc);
    }
    fr30_to_limbs(mul(rep, acc, fr30_const_one270()), out);
}

// The Horner step over the coefficients a[n - 1] .. a[0] with the multiplier z.
// form 0 (the quotient scans, fr30_mul_add): h = fr30_norm(fr30_add_raw(fr30_mul(h, z), c)), out[i] = fr30_to_limbs(h) after
//        coefficient i (n values: out[1..] is the quotient, out[0] the value).
// form 1 (cmb_steps): h = fr30_add_raw(fr30_mul(h, z), c) goes into the next product as it is; out = the one value
//        fr30_to_limbs(fr30_mul(h, zl)) for the closing multiplier zl.
// b != null is the WEAKENED variant of form 1: both a[i] and b[i] are added raw, a raw sum of three (never on a device).
void fre_horner(const uint32_t* a, const uint32_t* b, int n, const uint64_t* z_image, const uint64_t* zl_image, int form,
                uint32_t* out, uint64_t* report) {
    Rep rep = start(report);
    const Fr30 z = mult(z_image);
    Fr30 h = fr30_zero();
    for (int i = n - 1; i >= 0; i--) {
        h = add_raw(rep, mul(rep, h, z), load(rep, a + 8 * i));
        if (b) h = add_raw(rep, h, load(rep, b + 8 * i));
        if (form == 0) {
            h = norm(rep, h);
            fr30_to_limbs(h, out + 8 * i);
        }
    }
    if (form == 1) fr30_to_limbs(mul(rep, h, mult(zl_image)), out);
}

// k_ntt_pass on one tile of 2^m values x[r] (the values a DFT of the pass reads at stride N / 2^m): bit-reversed load, m
// radix-2 DIT stages (stage 0 without a product), out[r] = fr30_to_limbs(fr30_mul(v_r, last)).  roots: the 2^(m-1) multipliers
// w_(2^m)^j (one entry when m = 0); the stage twiddle w_(2h)^k is roots[k 2^(m-1-s)].
void fre_ntt(const uint32_t* x, int m, const uint64_t* roots, const uint64_t* last_image, uint32_t* out, uint64_t* report) {
    Rep rep = start(report);
    const uint32_t n = 1u << m;
    std::vector<Fr30> v(n), tw(m ? n / 2 : 1);
    for (size_t j = 0; j < tw.size(); j++) tw[j] = mult(roots + 4 * j);
    for (uint32_t r = 0; r < n; r++) {
        uint32_t pos = 0;
        for (int bit = 0; bit < m; bit++) pos |= ((r >> bit) & 1u) << (m - 1 - bit);
        v[pos] = load(rep, x + 8 * r);
    }
    for (int s = 0; s < m; s++) {
        const uint32_t h = 1u << s;
        for (uint32_t q = 0; q < n / 2; q++) {
            const uint32_t k = q & (h - 1), p0 = ((q >> s) << (s + 1)) + k, p1 = p0 + h;
            const Fr30 xv = v[p0];
            Fr30 y = v[p1];
            if (s) y = mul(rep, y, tw[(size_t)k << (m - 1 - s)]);
            v[p0] = add(rep, xv, y);
            v[p1] = sub(rep, xv, y);
        }
    }
    const Fr30 last = mult(last_image);
    for (uint32_t r = 0; r < n; r++) fr30_to_limbs(mul(rep, v[r], last), out + 8 * r);
}

// The sums of k_bary_partial and k_bary_finish over n = tiles * 1024 terms f_i m_i (m_i = w^i / (z - w^i) given as a
// multiplier): index tile * 1024 + j * 256 + t belongs to run t of the tile.  Run: four fr30_add, one product with one; tile: a
// tree over 256 runs, one product with one; finish: lane q adds the tiles q + 64 k, lane 0 adds the 64 lanes; out =
// fr30_to_limbs(acc x one x factor).
void fre_bary(const uint32_t* f, const uint64_t* ms, int tiles, const uint64_t* factor_image, uint32_t* out, uint64_t* report) {
    Rep rep = start(report);
    const Fr30 one = fr30_const_one270();
    std::vector<Fr30> partial(tiles);
    for (int tile = 0; tile < tiles; tile++) {
        Fr30 red[256];
        for (int t = 0; t < 256; t++) {
            Fr30 acc = fr30_zero();
            for (int j = 3; j >= 0; j--) {
                const size_t i = (size_t)tile * 1024 + j * 256 + t;
                acc = add(rep, acc, mul(rep, load(rep, f + 8 * i), mult(ms + 4 * i)));
            }
            red[t] = mul(rep, acc, one);
        }
        for (int o = 128; o > 0; o >>= 1)
            for (int t = 0; t < o; t++) red[t] = add(rep, red[t], red[t + o]);
        partial[tile] = mul(rep, red[0], one);
    }
    Fr30 lanes[64];
    for (int q = 0; q < 64; q++) {
        lanes[q] = fr30_zero();
        for (int k = q; k < tiles; k += 64) lanes[q] = add(rep, lanes[q], partial[k]);
    }
    Fr30 acc = lanes[0];
    for (int q = 1; q < 64; q++) acc = add(rep, acc, lanes[q]);
    fr30_to_limbs(mul(rep, mul(rep, acc, one), mult(factor_image)), out);
}

// k_vc_fr_sum's fold of one column: level 0 takes groups of at most `fold` consecutive rows, acc = fr30_add(acc, v x rho),
// and stores fr30_to_limbs(acc x one); the later levels add the stored canonical values the same way, without weights.
void fre_fold(const uint32_t* values, const uint64_t* rhos, int count, int fold, uint32_t* out, uint64_t* report) {
    Rep rep = start(report);
    const Fr30 one = fr30_const_one270();
    std::vector<uint32_t> cur(values, values + 8 * (size_t)count), next;
    bool weighted = true;
    do {
        const int groups = (count + fold - 1) / fold;
        next.assign(8 * (size_t)groups, 0);
        for (int g = 0; g < groups; g++) {
            Fr30 acc = fr30_zero();
            for (int q = g * fold; q < count && q < (g + 1) * fold; q++) {
                Fr30 v = load(rep, cur.data() + 8 * (size_t)q);
                if (weighted) v = mul(rep, v, mult(rhos + 4 * q));
                acc = add(rep, acc, v);
            }
            fr30_to_limbs(mul(rep, acc, one), next.data() + 8 * (size_t)g);
        }
        cur.swap(next);
        count = groups;
        weighted = false;
    } while (count > 1);
    memcpy(out, cur.data(), 32);
}

}  // extern "C"
