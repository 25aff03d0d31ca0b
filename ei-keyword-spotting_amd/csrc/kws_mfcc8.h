// kws_mfcc8.h -- what kws_mfcc8_kernel (kws_mfcc.hip) and its ragged form (kws_mfcc8_ragged_kernel, kws_ragged_kernels.hip) share besides
// kws_device.h: the DCT of both MFCC kernels, the eight-lanes-per-frame layout's constants and its LDS block.
#pragma once
#include "kws_device.h"
#include "kws_dct_tables.h"

// kf_bfly5 with m = 1 (kiss_fft.cpp:131-192): every product and sum in the reference's order
__device__ __forceinline__ void bfly5(cf &F0, cf &F1, cf &F2, cf &F3, cf &F4, cf t1, cf t2, cf t3, cf t4, cf ya, cf yb)
{
    const cf s0 = F0;
    const cf s1 = cmul(F1, t1), s2 = cmul(F2, t2), s3 = cmul(F3, t3), s4 = cmul(F4, t4);
    const cf s7 = cadd(s1, s4), s10 = csub(s1, s4), s8 = cadd(s2, s3), s9 = csub(s2, s3);
    float tt, a, b;
    tt = s7.r + s8.r; F0.r = F0.r + tt;
    tt = s7.i + s8.i; F0.i = F0.i + tt;
    cf s5, s6, s11, s12;
    a = s7.r * ya.r; b = s8.r * yb.r; s5.r = (s0.r + a) + b;
    a = s7.i * ya.r; b = s8.i * yb.r; s5.i = (s0.i + a) + b;
    a = s10.i * ya.i; b = s9.i * yb.i; s6.r = a + b;
    a = s10.r * ya.i; b = s9.r * yb.i; s6.i = (-a) - b;
    F1 = csub(s5, s6);
    F4 = cadd(s5, s6);
    a = s7.r * yb.r; b = s8.r * ya.r; s11.r = (s0.r + a) + b;
    a = s7.i * yb.r; b = s8.i * ya.r; s11.i = (s0.i + a) + b;
    a = s10.i * yb.i; b = s9.i * ya.i; s12.r = (-a) + b;
    a = s10.r * yb.i; b = s9.r * ya.i; s12.i = a - b;
    F2 = cadd(s11, s12);
    F3 = csub(s11, s12);
}

// numpy::dct2 of one frame (numpy.hpp:378-401 -> dct::transform, fast-dct-fft.cpp:37-80 -> kiss_fftr(NF)): v holds the NF
// log-mel energies; R receives the NF/2+1 spectrum points the transform reads.  The complex FFT of NF/2 points is
// kf_work's recursion unrolled: NF = 32 -> 16 = 4 x 4 (kf_bfly4, kf_bfly4); NF = 40 -> 20 = 4 x 5 (kf_bfly5 leaves of
// stride 4, then kf_bfly4 with m = 5).
template <int NF, typename Emit>
__device__ __forceinline__ void dct_spectrum(const float (&v)[NF], Emit emit)   // emit(i, R[i]), i = 0..NF/2
{
    constexpr int NC = NF / 2;
    // twiddles as literals (kws_dct_tables.h): every index below is a compile-time constant once the loops are unrolled.
    // From the plan's tables they are scalar loads whose registers get spilled and reloaded around every output.
    typedef KwsDctTab<NF> T;
    auto tw = [](int i) { cf c; c.r = T::tw_r[i]; c.i = T::tw_i[i]; return c; };
    auto stw = [](int i) { cf c; c.r = T::stw_r[i]; c.i = T::stw_i[i]; return c; };
    // even/odd reorder (in[i] = v[2i], in[NF-1-i] = v[2i+1]) read as NC complex points
    auto rin = [&](int i) { return (i < NC) ? v[2 * i] : v[2 * (NF - 1 - i) + 1]; };
    cf F[NC];
    if constexpr (NF == 32) {
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int n = q + 4 * j;                           // complex input index of leaf q
                F[4 * q + j].r = rin(2 * n);
                F[4 * q + j].i = rin(2 * n + 1);
            }
        const cf d0 = tw(0);
#pragma unroll
        for (int q = 0; q < 4; ++q) bfly4(F[4 * q], F[4 * q + 1], F[4 * q + 2], F[4 * q + 3], d0, d0, d0);
#pragma unroll
        for (int k = 0; k < 4; ++k)
            bfly4(F[k], F[k + 4], F[k + 8], F[k + 12], tw(k), tw(2 * k), tw(3 * k));
    } else {
        static_assert(NF == 40, "DCT sizes: 32, 40");
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int j = 0; j < 5; ++j) {
                const int n = q + 4 * j;
                F[5 * q + j].r = rin(2 * n);
                F[5 * q + j].i = rin(2 * n + 1);
            }
        const cf d0 = tw(0), ya = tw(4), yb = tw(8);   // tw[fstride*m], tw[2*fstride*m]
#pragma unroll
        for (int q = 0; q < 4; ++q) bfly5(F[5 * q], F[5 * q + 1], F[5 * q + 2], F[5 * q + 3], F[5 * q + 4], d0, d0, d0, d0, ya, yb);
#pragma unroll
        for (int k = 0; k < 5; ++k)
            bfly4(F[k], F[k + 5], F[k + 10], F[k + 15], tw(k), tw(2 * k), tw(3 * k));
    }
    // kiss_fftr split (kiss_fftr.cpp:84-119); every spectrum point is handed on as soon as it exists
    cf r0, rn;
    r0.r = F[0].r + F[0].i; r0.i = 0.0f;
    rn.r = F[0].r - F[0].i; rn.i = 0.0f;
    emit(0, r0);
    emit(NC, rn);
#pragma unroll
    for (int k = 1; k <= NC / 2; ++k) {
        cf fpk = F[k], fpnk;
        fpnk.r = F[NC - k].r; fpnk.i = -F[NC - k].i;
        cf f1k = cadd(fpk, fpnk), f2k = csub(fpk, fpnk);
        cf twv = cmul(f2k, stw(k - 1));
        cf lo, hi;
        lo.r = (f1k.r + twv.r) * 0.5f;
        lo.i = (f1k.i + twv.i) * 0.5f;
        hi.r = (f1k.r - twv.r) * 0.5f;
        hi.i = (twv.i - f1k.i) * 0.5f;
        if (k != NC - k) emit(k, lo);                              // k == ncfft/2: overwritten by the "ncfft-k" store
        emit(NC - k, hi);
    }
}

// PROF: development aid -- per-phase shader-clock totals of block 0 are written to prof_out (tools/gpu_phase_profile.py)
#define KWS_NPHASE 10
#define PH(i) do { if (PROF) { long long now_ = clock64(); ph[i] += now_ - tlast; tlast = now_; } } while (0)

// ---------------------------------------------------------------------------------------------------------
//  Kernel 1b: the same function -- same arithmetic, operation by operation -- on the spectral layout kws_fast_kernel introduced
//  (round 3): eight lanes own a frame and sixteen of its 128 complex points each, eight frames per pass, so that kf_bfly2 (m = 1),
//  kf_bfly4 (m = 2) and, after ONE exchange through LDS, kf_bfly4 m = 8 and m = 32 all run in registers (kiss_fft.cpp:15-84,
//  232-296); kws_mfcc_kernel's layout (32 lanes per frame, four points per lane) takes three exchanges per frame pair.  The lanes
//  of a frame swap the upper halves of their points for kiss_fftr's split (kiss_fftr.cpp:84-119); the power spectrum goes through
//  fp64 as in the reference (bin_power); a pass's eight power rows feed the frame energies (129 ordered additions, one lane per
//  frame) and the mel stage (lane = filter, its taps read from LDS).  DCT and cmvnw are kws_mfcc_kernel's.  int16 PCM, windows of 16
//  frames or more, one wave per window; float samples, short windows and the latency shape stay with kws_mfcc_kernel.
//  13 KB of LDS per wave (the exchange buffer, the power rows, the tail pass's buffers and cmvnw's tables share one region) + the mel taps.
// ---------------------------------------------------------------------------------------------------------
constexpr int KWS_M8_CHUNK = 8;      // frames per pass
constexpr int KWS_M8_XS = 144;       // floats per frame of the exchange buffer: 64 positions + 2 floats of padding per 8
constexpr int KWS_M8_PS = 136;       // floats per power row (129 bins): = 8 mod 64, the eight frames' stores of one bin cover the banks
constexpr int KWS_M8_MAP = 640;      // cmvnw's pad map sits behind its offset table (kws_mfcc_max_win: at most 640 offsets)
template <int NF, int NZ>
struct alignas(16) Mfcc8Smem {
    static constexpr int MELS = NF + 1;
    float r1[KWS_M8_CHUNK * KWS_M8_XS];
    float mel[kws_mel_rows(NF) * MELS];
    float energy[kws_mel_rows(NF)];
    // the mel filters' ascending-bin taps [tap][filter]: weight and bin (as an offset into a power row); taps beyond a filter's end have
    // weight 0 and read bin 0.  In registers they would stay live through the FFT (2 x 2 NZ values per lane) and be spilled.
    float tap_w[NZ * NF];
    int tap_b[NZ * NF];
};
static_assert(KWS_M8_CHUNK * KWS_M8_PS <= KWS_M8_CHUNK * KWS_M8_XS && 2 * KWS_M8_PS + 2 * KWS_ZF <= KWS_M8_CHUNK * KWS_M8_XS &&
              KWS_M8_MAP + KWS_MAXPROW <= KWS_M8_CHUNK * KWS_M8_XS, "everything that shares Mfcc8Smem::r1 fits");
static_assert(sizeof(Mfcc8Smem<32, KWS_MAXNZ>) <= 20 * 1024 && sizeof(Mfcc8Smem<40, KWS_MAXNZ>) <= 20 * 1024, "8 waves per CU need <= 20 KB LDS each");
