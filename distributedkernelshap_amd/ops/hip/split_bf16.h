// Exact three-way split of an fp32 value into bf16-representable pieces.
//
// hi + mid + lo == v exactly, and for every normal v each piece has its low
// 16 bits clear (so it is a bf16 value; its bf16 bit pattern is the upper half
// of the word): a float has 24 significant bits, and mask, subtract, mask,
// subtract hands each piece the next 8 of them.  Truncation (not
// round-to-nearest) is what keeps hi from rounding up to infinity, and makes
// every remainder exactly representable so each subtraction is exact.
// For a denormal v the remainder lo can keep bits below the bf16 range, which
// split_bf16_pattern drops (an error below 2^-133).
// Non-finite inputs are outside the contract (inf - inf gives NaN pieces).
#pragma once

#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SPLIT_BF16_HD __host__ __device__
#else
#define SPLIT_BF16_HD
#endif

struct SplitBf16 {
    float hi, mid, lo;
};

SPLIT_BF16_HD inline uint32_t split_bf16_bits(float v) {
    uint32_t u;
    memcpy(&u, &v, sizeof(u));
    return u;
}

SPLIT_BF16_HD inline float split_bf16_trunc(float v) {
    const uint32_t u = split_bf16_bits(v) & 0xFFFF0000u;
    float r;
    memcpy(&r, &u, sizeof(r));
    return r;
}

SPLIT_BF16_HD inline SplitBf16 split_bf16(float v) {
#if defined(__clang__)
    // the subtractions must not fuse with a multiply that produced v
#pragma clang fp contract(off)
#endif
    SplitBf16 s;
    s.hi = split_bf16_trunc(v);
    const float r1 = v - s.hi;          // exact: <= 16 significant bits left
    s.mid = split_bf16_trunc(r1);
    s.lo = r1 - s.mid;                  // exact: <= 8 significant bits left
    return s;
}

// bf16 bit pattern of a piece (its low 16 bits are clear for normal inputs)
SPLIT_BF16_HD inline uint16_t split_bf16_pattern(float piece) {
    return (uint16_t)(split_bf16_bits(piece) >> 16);
}
