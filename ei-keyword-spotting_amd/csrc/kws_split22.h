// kws_split22.h -- one fp32 value as the two binary16 halves the split-operand contraction multiplies (kws_fast.h: KwsFastBlock::hconv):
//     hi = half(y),  lo = half(y - hi)        -- hi + lo carries 22 significant bits of y.
// Host and device compile the same lines (tests/split22/split22_driver.cpp, run by tests/test_split22_host.py, runs them without a GPU).
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define KWS_SPLIT22_HD __host__ __device__
#else
#define KWS_SPLIT22_HD
#endif

// cmvnw's store of block 0's image (kws_fast.hip: fast_cmvn<..., SPLIT>): every clip's values are multiplied by the SAME power of two.  cmvnw's output is
// (x - window mean) / (window deviation + eps) with x a member of its own window of n rows, so |output| <= sqrt(n - 1); the plan takes this path for
// windows of up to KWS_SPLIT22_PRE_WIN rows: |output| < 16, |y| < 2^14 -- the headroom fast_split_trips leaves below binary16's 65504.
#define KWS_SPLIT22_PRE_EXP 10
#define KWS_SPLIT22_PRE_WIN 256
#define KWS_SPLIT22_MAX 65504.0f                 // the largest binary16; |y| >= 65520 converts to an infinity

// The halves of y = x s, s a POWER OF TWO (so that x s is exact and the fused form below is y - hi, bit for bit; on the device it is one mixed-precision
// multiply-add that reads hi as it is).  Returns d = y - hi, the value lo is converted from.  THE OVERFLOW RULE: nothing is clamped.  |y| >= 65520 (or a y
// that is not finite) gives an infinite or NaN hi and with it a d that is NOT FINITE; the caller folds d x 0 -- a NaN exactly then -- into the clip's guard
// sum, and a guard sum that is not a number hands the clip on to the exact kernels (kws_fast.hip: !(V x ... <= 1)).  The NaN is not left to travel through
// the network: fminf / fmaxf of the activation clamps drop a NaN operand, and a saturated +-inf would come out as a finite clamp bound.
KWS_SPLIT22_HD static inline float kws_split22(float x, float s, _Float16 *hi, _Float16 *lo)
{
    const _Float16 h = (_Float16)(x * s);
    const float d = __builtin_fmaf(x, s, -(float)h);        // exact for a finite h: the difference has at most 13 significant bits
    *hi = h;
    *lo = (_Float16)d;
    return d;
}
