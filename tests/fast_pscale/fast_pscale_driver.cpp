// fast_pscale_driver.cpp -- TEST INFRASTRUCTURE (tests/test_fast_pscale_host.py): csrc/kws_fast_scale.h -- the power-spectrum scale the fast kernel and its
// plan share, and the scaling of the mel tap weights the plan uploads -- run on the host.
//     fast_pscale_driver FFT_LENGTH IN OUT     IN: float32 weights (raw, native endian); OUT: the same weights through kws_fast_scale_taps
// Prints PSCALE <%a> BITS <hex> N <weights> SUBNORMAL <what kws_fast_scale_taps returned>.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "kws_fast_scale.h"

int main(int argc, char **argv)
{
    if (argc != 4) { fprintf(stderr, "usage: fast_pscale_driver FFT_LENGTH IN OUT\n"); return 2; }
    const int fft_length = atoi(argv[1]);
    const float inv_fft = (float)(1.0 / (double)(float)fft_length);      // KwsDspPlan::inv_fft (csrc/kws_plan.cpp)
    const float pscale = kws_fast_pscale(inv_fft);
    FILE *f = fopen(argv[2], "rb");
    if (!f) { perror(argv[2]); return 1; }
    std::vector<float> w;
    float buf[1024];
    size_t n;
    while ((n = fread(buf, sizeof(float), 1024, f)) > 0) w.insert(w.end(), buf, buf + n);
    fclose(f);
    const size_t bad = kws_fast_scale_taps(w.data(), w.size(), pscale);
    f = fopen(argv[3], "wb");
    if (!f) { perror(argv[3]); return 1; }
    if (fwrite(w.data(), sizeof(float), w.size(), f) != w.size()) { perror(argv[3]); return 1; }
    fclose(f);
    uint32_t b;
    memcpy(&b, &pscale, 4);
    printf("PSCALE %a BITS %08x N %zu SUBNORMAL %zu\n", (double)pscale, b, w.size(), bad);
    return 0;
}
