// kws_bfly_m2k1.h -- kf_bfly4 of the 128-point transform's m = 2 level at k = 1, written with the structure of its three twiddles.
// Host and device compile the same lines (tests/bfly_m2k1/bfly_m2k1_driver.cpp, run by tests/test_bfly_m2k1_host.py, compares them
// bit for bit with the plain butterfly without a GPU).
//
// KissFFT's table for nfft = 128 (cos / sin in double, cast to float; kiss_fft.cpp:351-357) holds
//     tw[16] = (3f3504f3, bf3504f3) = ( c, -c)          tw[32] = (248d3132, bf800000) = (e, -1)          tw[48] = (bf3504f3, bf3504f3) = (-c, -c)
// with ONE c = (float)cos(pi/4) and e = (float)cos(pi/2) = 6.123234e-17.  C_MUL (four separately rounded products, one difference,
// one sum) by such a twiddle has products that are negations of each other -- a product by -c is the negated product by c, a
// product by -1 the negated factor, both exact --, and x - (-y) is x + y in IEEE arithmetic, the sign of a zero included.  With
// P = f.r c and Q = f.i c:
//     f (c, -c)  = (P - (-Q), (-P) + Q)    = (P + Q, Q - P)
//     f (e, -1)  = (f.r e - (-f.i), (-f.r) + f.i e) = (f.r e + f.i, f.i e - f.r)
//     f (-c, -c) = ((-P) - (-Q), (-P) + (-Q)) = (Q - P, -P - Q)
// Every sum and difference has the plain butterfly's operand pair, so every bit of the result is the plain butterfly's (NaN payloads
// aside): six products instead of twelve, nothing contracted, nothing re-factorised.  The identity rests on the table's BIT PATTERNS:
// kws_bfly_m2k1_table_ok says whether a table has them, and a table that does not must not reach the helper (kws_fast_plan.cpp refuses
// the fast plan).
#pragma once
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define KWS_BFLY_HD __host__ __device__
#else
#define KWS_BFLY_HD
#endif

#pragma clang fp contract(off)

// C: a complex type with float members r, i (kws_device.h: cf).  c = tw[16].r, e = tw[32].r
template <class C>
KWS_BFLY_HD static inline void bfly4_m2k1(C &f0, C &f1, C &f2, C &f3, float c, float e)
{
    const float p1 = f1.r * c, q1 = f1.i * c, p3 = f3.r * c, q3 = f3.i * c;
    const float x2 = f2.r * e, y2 = f2.i * e;
    C s0, s1, s2;
    s0.r = p1 + q1;
    s0.i = q1 - p1;
    s1.r = x2 + f2.i;
    s1.i = y2 - f2.r;
    s2.r = q3 - p3;
    s2.i = -p3 - q3;
    // kf_bfly4's own tail (kiss_fft.cpp:38-84), as in bfly4
    C s5;
    s5.r = f0.r - s1.r; s5.i = f0.i - s1.i;
    f0.r = f0.r + s1.r; f0.i = f0.i + s1.i;
    C s3, s4;
    s3.r = s0.r + s2.r; s3.i = s0.i + s2.i;
    s4.r = s0.r - s2.r; s4.i = s0.i - s2.i;
    f2.r = f0.r - s3.r; f2.i = f0.i - s3.i;
    f0.r = f0.r + s3.r; f0.i = f0.i + s3.i;
    f1.r = s5.r + s4.i;
    f1.i = s5.i - s4.r;
    f3.r = s5.r - s4.i;
    f3.i = s5.i + s4.r;
}

// The three twiddles (re, im) of a table the helper may stand in for: (c, -c), (e, -1), (-c, -c) with one and the same c, compared as bits.
static inline bool kws_bfly_m2k1_table_ok(float t16r, float t16i, float t32r, float t32i, float t48r, float t48i)
{
    uint32_t b[6];
    const float v[6] = { t16r, t16i, t32r, t32i, t48r, t48i };
    memcpy(b, v, sizeof(b));
    const uint32_t c = b[0], nc = c ^ 0x80000000u;
    (void)t32r;                                    // e may be any finite value: the helper multiplies by it as the plain butterfly does
    return (c & 0x80000000u) == 0 && (c & 0x7f800000u) != 0x7f800000u && b[1] == nc && b[3] == 0xbf800000u && b[4] == nc && b[5] == nc;
}
