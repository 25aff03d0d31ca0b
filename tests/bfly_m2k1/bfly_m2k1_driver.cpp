// bfly_m2k1_driver.cpp -- TEST INFRASTRUCTURE (tests/test_bfly_m2k1_host.py): csrc/kws_bfly_m2k1.h -- the m = 2, k = 1 butterfly of the fast kernel's pass
// loop, the same lines host and device compile -- against the plain kf_bfly4 with the table's three twiddles, bit for bit, on the host.
//     bfly_m2k1_driver table            TW <i> <re bits> <im bits> (i = 16, 32, 48, recomputed as KissFFT builds its table), then OK <0|1> and
//                                       REJECT <n of n perturbed tables refused>
//     bfly_m2k1_driver random SEED N    N random cases (magnitudes 1e-30 .. 1e8, log-uniform, random signs)
//     bfly_m2k1_driver special          +-0, non-zero values, subnormals and +-inf in every combination over f1, f2, f3 (f0 cycles through the same set)
// The last two print CASES <n> MISMATCH <m> and up to eight BAD lines.  Two NaNs count as equal whatever their payloads.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "kws_bfly_m2k1.h"

struct cf { float r, i; };

// kws_device.h's cmul / bfly4 (kf_bfly4, kiss_fft.cpp:38-84; C_MUL: four products, one difference, one sum), for the host
static cf cmul(cf a, cf b)
{
    cf m;
    float rr = a.r * b.r, ii = a.i * b.i, ri = a.r * b.i, ir = a.i * b.r;
    m.r = rr - ii;
    m.i = ri + ir;
    return m;
}
static cf cadd(cf a, cf b) { cf c; c.r = a.r + b.r; c.i = a.i + b.i; return c; }
static cf csub(cf a, cf b) { cf c; c.r = a.r - b.r; c.i = a.i - b.i; return c; }
static void bfly4(cf &f0, cf &f1, cf &f2, cf &f3, cf t1, cf t2, cf t3)
{
    cf s0 = cmul(f1, t1), s1 = cmul(f2, t2), s2 = cmul(f3, t3);
    cf s5 = csub(f0, s1);
    f0 = cadd(f0, s1);
    cf s3 = cadd(s0, s2), s4 = csub(s0, s2);
    f2 = csub(f0, s3);
    f0 = cadd(f0, s3);
    f1.r = s5.r + s4.i;
    f1.i = s5.i - s4.r;
    f3.r = s5.r - s4.i;
    f3.i = s5.i + s4.r;
}

static uint32_t bits(float v) { uint32_t b; memcpy(&b, &v, 4); return b; }
static float from_bits(uint32_t b) { float v; memcpy(&v, &b, 4); return v; }

static cf tw[3];                                   // tw[16], tw[32], tw[48] of the 128-point table
static void make_table()
{
    for (int m = 1; m <= 3; m++) {                 // kiss_fft.cpp:351-357 (csrc/kws_model.cpp: h_twiddles)
        const double pi = 3.141592653589793238462643383279502884197169399375105820974944;
        const double phase = -2 * pi * (16 * m) / 128;
        tw[m - 1].r = (float)cos(phase);
        tw[m - 1].i = (float)sin(phase);
    }
}

static long n_cases = 0, n_bad = 0;
static void check(const float in[8])
{
    cf a[4], b[4];
    for (int k = 0; k < 4; k++) { a[k].r = b[k].r = in[2 * k]; a[k].i = b[k].i = in[2 * k + 1]; }
    bfly4(a[0], a[1], a[2], a[3], tw[0], tw[1], tw[2]);
    bfly4_m2k1(b[0], b[1], b[2], b[3], tw[0].r, tw[1].r);
    bool same = true;
    for (int k = 0; k < 4; k++) {
        const float x[2] = { a[k].r, a[k].i }, y[2] = { b[k].r, b[k].i };
        for (int c = 0; c < 2; c++) same = same && (bits(x[c]) == bits(y[c]) || (std::isnan(x[c]) && std::isnan(y[c])));
    }
    n_cases++;
    if (!same && n_bad++ < 8) {
        printf("BAD in");
        for (int k = 0; k < 8; k++) printf(" %08x", bits(in[k]));
        printf(" bfly4");
        for (int k = 0; k < 4; k++) printf(" %08x %08x", bits(a[k].r), bits(a[k].i));
        printf(" m2k1");
        for (int k = 0; k < 4; k++) printf(" %08x %08x", bits(b[k].r), bits(b[k].i));
        printf("\n");
    }
}

static uint64_t rng_state;
static uint64_t rng()                              // xorshift64*
{
    rng_state ^= rng_state >> 12; rng_state ^= rng_state << 25; rng_state ^= rng_state >> 27;
    return rng_state * 0x2545F4914F6CDD1DULL;
}
static double uni() { return (double)(rng() >> 11) * (1.0 / 9007199254740992.0); }

int main(int argc, char **argv)
{
    make_table();
    const char *mode = argc > 1 ? argv[1] : "";
    if (!strcmp(mode, "table")) {
        for (int m = 0; m < 3; m++) printf("TW %d %08x %08x\n", 16 * (m + 1), bits(tw[m].r), bits(tw[m].i));
        printf("OK %d\n", (int)kws_bfly_m2k1_table_ok(tw[0].r, tw[0].i, tw[1].r, tw[1].i, tw[2].r, tw[2].i));
        // a table one bit off in any of the five components the identity rests on is refused
        int refused = 0, tried = 0;
        for (int k = 0; k < 6; k++) {
            if (k == 2) continue;                  // tw[32].r = e is multiplied by as it is
            float v[6] = { tw[0].r, tw[0].i, tw[1].r, tw[1].i, tw[2].r, tw[2].i };
            v[k] = from_bits(bits(v[k]) ^ 1u);
            tried++;
            refused += !kws_bfly_m2k1_table_ok(v[0], v[1], v[2], v[3], v[4], v[5]);
        }
        printf("REJECT %d of %d\n", refused, tried);
        return 0;
    }
    if (!strcmp(mode, "random") && argc > 3) {
        rng_state = strtoull(argv[2], nullptr, 10) * 0x9E3779B97F4A7C15ULL + 1;
        const long n = atol(argv[3]);
        for (long c = 0; c < n; c++) {
            float in[8];
            for (int k = 0; k < 8; k++) {
                // 1e-30 .. 1e8, log-uniform; every fourth case keeps all eight values within a factor 16 of each other (sums that cancel)
                const double e = (c & 3) ? -30.0 + 38.0 * uni() : -30.0 + 36.0 * (double)((c >> 2) % 977) / 976.0 + 1.2 * uni();
                const double v = pow(10.0, e) * (0.5 + 0.5 * uni());
                in[k] = (float)((rng() & 1) ? -v : v);
            }
            check(in);
        }
    } else if (!strcmp(mode, "special")) {
        const float sub = from_bits(1u), sub2 = from_bits(0x00400123u), inf = INFINITY;
        const float xs[3] = { 1.5f, 3.4e7f, 2.0e-30f };
        for (int xi = 0; xi < 3; xi++) {
            const float x = xs[xi];
            const float set[10] = { 0.0f, -0.0f, x, -x, sub, -sub, sub2, -sub2, inf, -inf };
            const int ns = xi == 0 ? 10 : 6;       // the full set once (10^6 cases), +-0 / +-x / +-smallest subnormal for the other magnitudes
            long combos = 1;
            for (int k = 0; k < 6; k++) combos *= ns;
            for (long c = 0; c < combos; c++) {
                float in[8];
                long t = c;
                for (int k = 2; k < 8; k++) { in[k] = set[t % ns]; t /= ns; }
                in[0] = set[c % ns]; in[1] = set[(c / 7) % ns];
                check(in);
            }
        }
        // every +-0 combination over all eight components
        for (int c = 0; c < 256; c++) {
            float in[8];
            for (int k = 0; k < 8; k++) in[k] = (c >> k) & 1 ? -0.0f : 0.0f;
            check(in);
        }
        // one component of a point zero (either sign), the other not: every point, every placement, f0 non-zero and zero
        const float nz[4] = { 1.0f, -7.25f, 1.0e-20f, -3.0e7f };
        for (int c = 0; c < 4 * 4 * 4 * 4 * 4 * 4 * 4; c++) {
            float in[8];
            int t = c;
            for (int k = 0; k < 4; k++) {
                const int place = t & 3; t >>= 2;  // which component is the zero, and its sign
                const float v = nz[(c + k) & 3], z = (place & 2) ? -0.0f : 0.0f;
                in[2 * k] = (place & 1) ? z : v;
                in[2 * k + 1] = (place & 1) ? v : z;
            }
            for (int k = 0; k < 3; k++) { if ((t & 3) == 3) { in[2 * k + 2] = nz[k]; in[2 * k + 3] = nz[k + 1]; } t >>= 2; }
            check(in);
        }
    } else {
        fprintf(stderr, "usage: bfly_m2k1_driver table | random SEED N | special\n");
        return 2;
    }
    printf("CASES %ld MISMATCH %ld\n", n_cases, n_bad);
    return 0;
}
