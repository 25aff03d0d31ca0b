// kws_fast_scale.h -- where the fast kernel's power-spectrum scale lives.  Host and device compile the same lines
// (tests/fast_pscale/fast_pscale_driver.cpp, run by tests/test_fast_pscale_host.py, runs them without a GPU).
//
// The reference's power spectrum is |X|^2 / fft_length on samples scaled by 2^-15; the kernel transforms UNSCALED int16 samples and
// its real-transform split leaves twice the reference's bins, so a power needs the factor
//     pscale = (1 / fft_length) x 2^-30 x 1/4                     (2^-40 for the only length the kernel serves, 256),
// a power of two (the plan refuses any other fft_length).  The kernel's power rows have linear consumers only -- the mel dot products
// against tap_w1 / tap_w2 and the frame-energy sum -- so the factor is not applied per bin: the plan uploads the tap weights multiplied by
// it (kws_fast_scale_taps) and the kernel multiplies a frame's energy by it once, behind its lane reduction.
//
// WHY NO BIT MOVES.  Multiplying by a power of two commutes with every rounding as long as no value leaves the normal range, and an exact
// zero stays an exact zero (the == 0 tests see the same thing).  Unscaled: a split output is at most ~4.7e7 for int16 input, a power at
// most ~4.4e15, a frame's sum at most ~6e17, a mel sum no larger -- far from overflow.  At the other end the only value the move could
// change is a scaled power that WAS subnormal where it used to be rounded per bin: a non-zero unscaled power below 2^-86 = 1.3e-26, a bin
// below 1e-13 of an int16 step.  Bins of audio are >= ~1e-18 in power before the 2^-40; only the exact-cancellation residues of a constant
// input come near that floor (a product by the table's cos(pi/2) = 6.1e-17 that nothing else is added to), twenty orders of magnitude
// below the same frame's other bins and a subnormal's last place (1.4e-45) in the mel sum they enter.  The scaled weights (mel weights
// are >= ~1e-7 where they are not zero) are >= ~1e-19, normal: every product xv x w inside the mel sum's multiply-add is the old
// product, exactly.  (kws_fast_scale_taps reports a weight that would come out subnormal, and the plan refuses it.)
#pragma once
#include <stddef.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define KWS_FAST_SCALE_HD __host__ __device__
#else
#define KWS_FAST_SCALE_HD
#endif

// inv_fft = KwsDspPlan::inv_fft
KWS_FAST_SCALE_HD static inline float kws_fast_pscale(float inv_fft) { return inv_fft * (1.0f / 1073741824.0f) * 0.25f; }

// w[i] *= pscale in place; returns how many non-zero weights came out smaller than the smallest normal float (0: the scaling is exact)
static inline size_t kws_fast_scale_taps(float *w, size_t n, float pscale)
{
    size_t bad = 0;
    for (size_t i = 0; i < n; i++) {
        if (w[i] == 0.0f) continue;
        w[i] *= pscale;
        const float a = w[i] < 0.0f ? -w[i] : w[i];
        if (!(a >= 1.17549435e-38f)) bad++;
    }
    return bad;
}
