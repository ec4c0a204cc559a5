// rcdc_p1305.h -- Poly1305 arithmetic mod p = 2^130 - 5 on five 26-bit limbs
// with lazy carries: the one copy, for the device (rcdc_aead.hip) and the host
// (the key tables of rcdc_family_plans.h; tools/family_plans_check.cpp runs
// every function here against Python integers, tests/test_p1305_host.py).
//
// A P26 stands for sum h[k] * 2^(26 k).  "Canonical" limbs are below 2^26; a
// lazy limb holds more, and the value may be any representative mod p.  Each
// function states, as numbers, what it takes (entry) and what it leaves
// (exit); a caller owes the entry bound, and the host tests run every function
// at it.
//
// The limb contracts in one place:
//   tables (rpow, r2j: the b of pmul)   every limb < 2^26
//   accumulator into pmul (a)           every limb < 2^28
//   out of pmul                         h1 < 2^26 + 2^7, the others < 2^26
//   a message block (pblock)            h0..h3 < 2^26, h4 < 2^25
//   into pnorm, pfull                   every limb < 2^31
//   out of pnorm                        h1 <= 2^26, the others < 2^26
//   out of pfull, into ptag             every limb < 2^26, value < 2^130
// The Horner step pmul(acc, R) + pblock stays below 2^27 + 2^7 < 2^28; sums of
// two pnorm results (the wave reduction, the units of a blob) stay below 2^28.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define RCDC_P1305_FN __host__ __device__ __forceinline__
#else
#define RCDC_P1305_FN inline
#endif

namespace rcdc {
namespace p1305 {

struct P26 {
    uint32_t h[5];
};

// a * b mod 2^130 - 5.
// Entry: limbs of a < 2^28, limbs of b < 2^26 (a table row).  Then each of the
// five sums is at most 21 * 2^28 * 2^26 + a carry < 2^59: no 64-bit overflow.
// Exit: h0, h2, h3, h4 < 2^26; h1 < 2^26 + 2^7 (the wrapped top carry is at
// most 5 * (5 * 2^28 + 10) < 2^33, of which 2^7 reaches h1).
RCDC_P1305_FN P26 pmul(const P26 &a, const uint32_t *b) {
    const uint64_t b0 = b[0], b1 = b[1], b2 = b[2], b3 = b[3], b4 = b[4];
    const uint64_t s1 = b1 * 5, s2 = b2 * 5, s3 = b3 * 5, s4 = b4 * 5;
    const uint64_t a0 = a.h[0], a1 = a.h[1], a2 = a.h[2], a3 = a.h[3], a4 = a.h[4];
    uint64_t d0 = a0 * b0 + a1 * s4 + a2 * s3 + a3 * s2 + a4 * s1;
    uint64_t d1 = a0 * b1 + a1 * b0 + a2 * s4 + a3 * s3 + a4 * s2;
    uint64_t d2 = a0 * b2 + a1 * b1 + a2 * b0 + a3 * s4 + a4 * s3;
    uint64_t d3 = a0 * b3 + a1 * b2 + a2 * b1 + a3 * b0 + a4 * s4;
    uint64_t d4 = a0 * b4 + a1 * b3 + a2 * b2 + a3 * b1 + a4 * b0;
    P26 r;
    d1 += d0 >> 26;
    r.h[0] = (uint32_t)d0 & 0x3ffffff;
    d2 += d1 >> 26;
    r.h[1] = (uint32_t)d1 & 0x3ffffff;
    d3 += d2 >> 26;
    r.h[2] = (uint32_t)d2 & 0x3ffffff;
    d4 += d3 >> 26;
    r.h[3] = (uint32_t)d3 & 0x3ffffff;
    const uint64_t c = d4 >> 26;
    r.h[4] = (uint32_t)d4 & 0x3ffffff;
    const uint64_t t0 = (uint64_t)r.h[0] + c * 5;
    r.h[0] = (uint32_t)t0 & 0x3ffffff;
    r.h[1] += (uint32_t)(t0 >> 26);
    return r;
}

// One carry pass with the wrap 2^130 = 5; the value mod p stays.
// Entry: every limb < 2^31 (a carry is then < 2^5 + 1, no 32-bit overflow).
// Exit: h0, h2, h3, h4 < 2^26; h1 <= 2^26 (the wrap adds at most 5 * 32 to
// h0, so its carry into h1 is 0 or 1).  The value may still be p or more.
RCDC_P1305_FN void pnorm(P26 &a) {
    uint32_t c;
    c = a.h[0] >> 26; a.h[0] &= 0x3ffffff; a.h[1] += c;
    c = a.h[1] >> 26; a.h[1] &= 0x3ffffff; a.h[2] += c;
    c = a.h[2] >> 26; a.h[2] &= 0x3ffffff; a.h[3] += c;
    c = a.h[3] >> 26; a.h[3] &= 0x3ffffff; a.h[4] += c;
    c = a.h[4] >> 26; a.h[4] &= 0x3ffffff; a.h[0] += c * 5;
    c = a.h[0] >> 26; a.h[0] &= 0x3ffffff; a.h[1] += c;
}

// The 16-byte message block w (4 little-endian words) plus 2^(8 k), k the
// block's byte count (16: the 2^128 bit).
// Entry: k <= 16; bytes of w at and after k may hold anything.
// Exit: h0..h3 < 2^26, h4 < 2^25; the value is below 2^129.
RCDC_P1305_FN P26 pblock(const uint32_t w[4], uint32_t k) {
    uint32_t x[4] = {w[0], w[1], w[2], w[3]};
    uint32_t hib = 0;
    if (k < 16) {  // partial final block: bytes >= k are zero, then the 1 byte
        for (int i = 0; i < 4; i++) {
            const int lo = 4 * i;
            if ((int)k <= lo) x[i] = 0;
            else if ((int)k < lo + 4) x[i] &= (1u << (8 * (k - lo))) - 1u;
        }
        x[k >> 2] |= 1u << (8 * (k & 3));
    } else {
        hib = 1;
    }
    P26 m;
    m.h[0] = x[0] & 0x3ffffff;
    m.h[1] = ((x[0] >> 26) | (x[1] << 6)) & 0x3ffffff;
    m.h[2] = ((x[1] >> 20) | (x[2] << 12)) & 0x3ffffff;
    m.h[3] = ((x[2] >> 14) | (x[3] << 18)) & 0x3ffffff;
    m.h[4] = (x[3] >> 8) | (hib << 24);
    return m;
}

// Carry-propagate and wrap until every limb is below 2^26 and the value is
// below 2^130.
// Entry: every limb < 2^31.  The first pass leaves at most 2^130 + 5 * 32, the
// second wraps what is left of that, the last chain carries it up.
// Exit: every limb < 2^26, so the value is < 2^130 (it may be p .. 2^130 - 1).
RCDC_P1305_FN void pfull(P26 &a) {
    for (int rep = 0; rep < 2; rep++) {
        for (int j = 0; j < 4; j++) {
            a.h[j + 1] += a.h[j] >> 26;
            a.h[j] &= 0x3ffffff;
        }
        const uint32_t c = a.h[4] >> 26;
        a.h[4] &= 0x3ffffff;
        a.h[0] += c * 5;
    }
    for (int j = 0; j < 4; j++) {
        a.h[j + 1] += a.h[j] >> 26;
        a.h[j] &= 0x3ffffff;
    }
}

// The tag: (h mod p + s) mod 2^128 as 16 little-endian bytes, s = shi * 2^64 +
// slo.
// Entry: every limb of h < 2^26 (pfull's exit: h < 2^130 < 2 p, so one
// conditional subtraction reduces it).
RCDC_P1305_FN void ptag(P26 h, uint64_t slo, uint64_t shi, uint8_t tag[16]) {
    // h mod p: h - p if h >= p
    uint32_t g[5];
    uint32_t c = 5;
    for (int j = 0; j < 5; j++) {
        const uint32_t t = h.h[j] + c;
        g[j] = t & 0x3ffffff;
        c = t >> 26;
    }
    if (c) {  // h + 5 >= 2^130
        for (int j = 0; j < 5; j++) h.h[j] = g[j];
    }
    const uint64_t lo = (uint64_t)h.h[0] | (uint64_t)h.h[1] << 26 | (uint64_t)h.h[2] << 52;
    const uint64_t hi = (uint64_t)(h.h[2] >> 12) | (uint64_t)h.h[3] << 14 | (uint64_t)h.h[4] << 40;
    const uint64_t tlo = lo + slo;
    const uint64_t thi = hi + shi + (tlo < lo ? 1 : 0);
    for (int j = 0; j < 8; j++) {
        tag[j] = (uint8_t)(tlo >> (8 * j));
        tag[8 + j] = (uint8_t)(thi >> (8 * j));
    }
}

}  // namespace p1305
}  // namespace rcdc
