/*
 * gx_dec128.h — 128-bit integer helpers for the exact DECIMAL SUM/AVG
 * aggregates (GX_AGG_SUM_DEC / GX_AGG_AVG_DEC) and the general 40-B
 * DecimalStructure record (polardbx-common DecimalTypeBase.java:61-65,
 * 101-102: roundUp(integers) base-1e9 integer words, most significant first,
 * then roundUp(fractions) fraction words, the last one left-aligned;
 * integers@36, fractions@37, derivedFractions@38, isNeg@39).
 *
 * Plain C++ over two u64 halves, compiled for host and device alike: no
 * __int128 (its division is a library call device code does not have), and
 * every division is a 64-by-32-bit step over 32-bit limbs, or a shift-
 * subtract loop where the divisor does not fit 32 bits.
 */
#ifndef GX_DEC128_H
#define GX_DEC128_H

#include <stdint.h>

#if defined(__HIPCC__)
#define GX_HD __host__ __device__
#else
#define GX_HD
#endif

struct gx_u128 {
    unsigned long long lo, hi;
};

/* fences of the DECIMAL-input decode (sticky bits of one device word) */
#define GX_DEC_FENCE_FRAC  1u /* fractions > the aggregate's scale */
#define GX_DEC_FENCE_WORDS 2u /* more than 9 words in the record */
#define GX_DEC_FENCE_MAG   4u /* |value x 10^scale| >= 10^29 */

/* 10^29: DECIMAL inputs stay below it, so 2^30 of them stay below 2^127 */
#define GX_DEC_1E29_HI 0x1431e0faeull
#define GX_DEC_1E29_LO 0x6d7217caa0000000ull

GX_HD static inline uint32_t gx_pow10_u32(int e) { /* 0 <= e <= 9 */
    uint32_t p = 1;
    for (int i = 0; i < e; i++) p *= 10u;
    return p;
}

GX_HD static inline bool gx_u128_is_zero(gx_u128 a) {
    return (a.lo | a.hi) == 0ull;
}
GX_HD static inline bool gx_u128_ge(gx_u128 a, unsigned long long hi,
                                    unsigned long long lo) {
    return a.hi > hi || (a.hi == hi && a.lo >= lo);
}
GX_HD static inline gx_u128 gx_u128_neg(gx_u128 a) { /* two's complement */
    gx_u128 r;
    r.lo = ~a.lo + 1ull;
    r.hi = ~a.hi + (r.lo == 0ull ? 1ull : 0ull);
    return r;
}

/* a * m + add (mod 2^128) */
GX_HD static inline gx_u128 gx_u128_mul_add_u32(gx_u128 a, uint32_t m,
                                                uint32_t add) {
    const unsigned long long p0 = (a.lo & 0xFFFFFFFFull) * m + add;
    const unsigned long long p1 = (a.lo >> 32) * m + (p0 >> 32);
    gx_u128 r;
    r.lo = (p1 << 32) | (p0 & 0xFFFFFFFFull);
    r.hi = a.hi * m + (p1 >> 32);
    return r;
}

/* a /= d, returns a % d: four 64-by-32-bit steps, most significant first */
GX_HD static inline uint32_t gx_u128_divmod_u32(gx_u128 &a, uint32_t d) {
    unsigned long long cur, rem;
    cur = a.hi >> 32;
    const unsigned long long q3 = cur / d; rem = cur % d;
    cur = (rem << 32) | (a.hi & 0xFFFFFFFFull);
    const unsigned long long q2 = cur / d; rem = cur % d;
    cur = (rem << 32) | (a.lo >> 32);
    const unsigned long long q1 = cur / d; rem = cur % d;
    cur = (rem << 32) | (a.lo & 0xFFFFFFFFull);
    const unsigned long long q0 = cur / d; rem = cur % d;
    a.hi = (q3 << 32) | q2;
    a.lo = (q1 << 32) | q0;
    return (uint32_t)rem;
}

/* a /= d, returns a % d, d != 0: limb steps when d fits 32 bits, else
 * restoring shift-subtract (the remainder may need a 65th bit: `top`) */
GX_HD static inline unsigned long long gx_u128_divmod_u64(
    gx_u128 &a, unsigned long long d) {
    if ((d >> 32) == 0ull) return gx_u128_divmod_u32(a, (uint32_t)d);
    gx_u128 q;
    q.lo = 0ull; q.hi = 0ull;
    unsigned long long rem = 0ull;
    for (int i = 127; i >= 0; i--) {
        const unsigned long long top = rem >> 63;
        const unsigned long long bit =
            i >= 64 ? (a.hi >> (i - 64)) & 1ull : (a.lo >> i) & 1ull;
        rem = (rem << 1) | bit;
        if (top || rem >= d) {
            rem -= d;
            if (i >= 64) q.hi |= 1ull << (i - 64);
            else q.lo |= 1ull << i;
        }
    }
    a = q;
    return rem;
}

/* Decode one 40-B DecimalStructure record to |value| x 10^scale (scale 0..9)
 * and its sign. Returns 0, or the fence that rejects the value (then *mag
 * is unspecified). Reads only the record's own 40 bytes whatever its
 * integers/fractions bytes say. */
GX_HD static inline uint32_t gx_dec40_to_u128(const uint8_t *p, int scale,
                                              gx_u128 *mag, bool *neg) {
    const uint32_t *w = (const uint32_t *)p;
    const int iw = ((int)p[36] + 8) / 9;
    const int fractions = (int)p[37];
    const int fw = (fractions + 8) / 9;
    *neg = p[39] != 0;
    if (iw + fw > 9) return GX_DEC_FENCE_WORDS;
    if (fractions > scale) return GX_DEC_FENCE_FRAC; /* so fw <= 1 */
    gx_u128 acc;
    acc.lo = 0ull; acc.hi = 0ull;
    for (int k = 0; k < iw; k++) {
        /* acc < 10^29 here, so acc x 10^9 + w < 10^38 + 2^32 < 2^127 */
        acc = gx_u128_mul_add_u32(acc, 1000000000u, w[k]);
        if (gx_u128_ge(acc, GX_DEC_1E29_HI, GX_DEC_1E29_LO))
            return GX_DEC_FENCE_MAG;
    }
    /* the fraction word holds frac x 10^(9 - fractions): a multiple of
     * 10^(9 - scale), the division is exact */
    const uint32_t fr = fw ? w[iw] / gx_pow10_u32(9 - scale) : 0u;
    acc = gx_u128_mul_add_u32(acc, gx_pow10_u32(scale), fr);
    if (gx_u128_ge(acc, GX_DEC_1E29_HI, GX_DEC_1E29_LO))
        return GX_DEC_FENCE_MAG;
    *mag = acc;
    return 0u;
}

/* Write |value| x 10^scale = mag as a 40-B record (p 8-byte aligned):
 * integer words base 1e9, most significant first, at least one; one
 * fraction word frac x 10^(9-scale); integers = 9 x words; fractions =
 * derivedFractions = scale; isNeg only for a nonzero value. Any mag < 2^128
 * has at most 39 digits: 5 integer words + 1 fraction word. */
GX_HD static inline void gx_u128_to_dec40(gx_u128 mag, bool neg, int scale,
                                          uint8_t *p) {
    for (int k = 0; k < 5; k++) ((unsigned long long *)p)[k] = 0ull;
    const bool zero = gx_u128_is_zero(mag);
    const uint32_t frac = gx_u128_divmod_u32(mag, gx_pow10_u32(scale));
    /* static indices only: the words stay in registers */
    uint32_t iwv[5];
    int n = 1;
#pragma unroll
    for (int i = 0; i < 5; i++) {
        iwv[i] = gx_u128_divmod_u32(mag, 1000000000u);
        if (iwv[i] != 0u) n = i + 1;
    }
    uint32_t *w = (uint32_t *)p;
#pragma unroll
    for (int i = 0; i < 5; i++)
        if (i < n) w[n - 1 - i] = iwv[i];
    w[n] = frac * gx_pow10_u32(9 - scale);
    p[36] = (uint8_t)(9 * n);
    p[37] = (uint8_t)scale;
    p[38] = (uint8_t)scale;
    p[39] = (neg && !zero) ? 1 : 0;
}

/* AVG: round_half_up(|sum| x 10^-scale / count, 4) as a scale-4 magnitude,
 * scale <= 4, count != 0 (SpecificType2DecimalAvg.writeResultTo:93-114 with
 * DEFAULT_DIV_PRECISION_INCREMENT = 4, magnitude rounding):
 * q x 10^(4-scale) + round_half_up(r x 10^(4-scale) / count). */
GX_HD static inline gx_u128 gx_dec_avg4(gx_u128 mag, unsigned long long count,
                                        int scale) {
    const uint32_t m = gx_pow10_u32(4 - scale);
    gx_u128 t;
    t.lo = gx_u128_divmod_u64(mag, count); /* mag = q, t = r < count */
    t.hi = 0ull;
    t = gx_u128_mul_add_u32(t, m, 0u);
    const unsigned long long r2 = gx_u128_divmod_u64(t, count); /* t < m */
    uint32_t q2 = (uint32_t)t.lo;
    if (r2 >= count - r2) q2++; /* 2 x r2 >= count without overflow */
    return gx_u128_mul_add_u32(mag, m, q2);
}

#endif /* GX_DEC128_H */
