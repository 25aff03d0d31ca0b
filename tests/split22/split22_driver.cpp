// split22_driver.cpp -- TEST INFRASTRUCTURE (tests/test_split22_host.py): the conversion the fast kernel's cmvnw stores its features with (csrc/kws_split22.h,
// the same lines host and device compile), run on the host.  Prints one line per probe:
//     SPLIT <y as %a> hi <%a> lo <%a> d <%a> hi_finite <0|1> d_finite <0|1> flag_is_nan <0|1>
// flag = 0 + d x 0, what the kernel adds to a clip's guard sum: NaN exactly when the value left binary16's range.
#include <cmath>
#include <cstdio>
#include <cstdlib>

#include "kws_split22.h"

static void probe(float x, float s)
{
    _Float16 hi, lo;
    const float d = kws_split22(x, s, &hi, &lo);
    const float flag = __builtin_fmaf(d, 0.0f, 0.0f);
    printf("SPLIT %a hi %a lo %a d %a hi_finite %d d_finite %d flag_is_nan %d\n", (double)(x * s), (double)(float)hi, (double)(float)lo, (double)d,
           (int)std::isfinite((float)hi), (int)std::isfinite(d), (int)std::isnan(flag));
}

int main(int argc, char **argv)
{
    const float s = (float)(1 << KWS_SPLIT22_PRE_EXP);
    printf("SCALE %a MAX %a WIN %d\n", (double)s, (double)KWS_SPLIT22_MAX, KWS_SPLIT22_PRE_WIN);
    // every argument: a value of y = x s as a C99 hexadecimal float (or inf / nan); x = y / s is exact for the finite ones given here
    for (int i = 1; i < argc; i++) probe(strtof(argv[i], nullptr) / s, s);
    return 0;
}
