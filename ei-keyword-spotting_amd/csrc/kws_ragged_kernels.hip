// kws_ragged_kernels.hip -- the kernels of kws_run_classifier_ragged_device (kws_ragged.cpp): kws_mfcc8_ragged_kernel, the ragged form of
// kws_mfcc8_kernel (frame count, length, base address and pad map per clip; the DCT, the layout constants and the LDS block are shared:
// kws_mfcc8.h), and the two copy kernels of the staging / grouped routes.  Built without the SLP vectoriser, as kws_mfcc.hip is (see the Makefile).
#include "kws_mfcc8.h"
#include "kws_ragged.h"

// kws_mfcc8_kernel (kws_mfcc.hip) with cmvnw, for clips of their own lengths: the same arithmetic, operation by operation, in the same
// order -- the spectral passes, the tail pass, the DCT and cmvnw below are that kernel's, line for line -- but what it takes from the plan
// once per launch is taken here per clip from R.clips[clip]: nfr, the number of passes, the tail-pass rule, prow, the wrap sample
// x[length - 1] and the pad map (row nfr of R.pad_maps).  All of these are wave-uniform (the descriptor is one 16-byte scalar load).  Output
// rows are out_stride values apart (the model's feature count); the values behind the nfr x ncep that fit are written as +0.0f /
// quantise(0): the reference's calloc'd matrix (ei_run_classifier.h: features_matrix).  A change to either kernel's arithmetic belongs in
// both; tests/test_gpu_ragged.py holds them bit-identical on full-length clips.
template <int NZ, int NF, bool WIDE, int OCC>
__global__ __launch_bounds__(KWS_WAVE, OCC) void kws_mfcc8_ragged_kernel(KwsDspPlan P, KwsRaggedArgs R, int n_clips, float *__restrict__ features,
                                                                         int8_t *__restrict__ q_out, float in_scale, int in_zp, int out_stride)
{
    constexpr int MELS = NF + 1, NCEPT = NF / 2 + 1, PS = KWS_M8_PS, XS = KWS_M8_XS;
    __shared__ Mfcc8Smem<NF, NZ> sm;
    const int lane = threadIdx.x;
    float *const xw = sm.r1, *const pw = sm.r1;                        // the FFT's exchange buffer; the power rows reuse it
    int *const offt = (int *)sm.r1, *const sm_map = (int *)sm.r1 + KWS_M8_MAP;   // cmvnw's tables: the spectral buffers are dead by then
    const int ncep = P.n_cepstral;
    const float pre_cof = P.pre_cof, inv_fft = P.inv_fft;
    const int frame_stride = P.frame_stride;
    if (lane < NF) {
        const int s0 = P.filt_start[lane], e0 = P.filt_start[lane + 1];
#pragma unroll
        for (int n = 0; n < NZ; ++n) {
            const bool on = s0 + n < e0;
            sm.tap_b[n * NF + lane] = on ? P.filt_bin[s0 + n] : 0;
            sm.tap_w[n * NF + lane] = on ? P.filt_w[s0 + n] : 0.0f;
        }
    }
    WAVE_SYNC();

    int touched_next = 0;
    for (int clip = blockIdx.x; clip < n_clips; clip += gridDim.x) {
        // this clip's descriptor -- one 16-byte scalar load (clip is wave-uniform) -- and what kws_mfcc8_kernel takes from the plan
        const KwsRaggedClip rc = R.clips[clip];
        const int nfr = rc.frames, n_samples = rc.length, prow = nfr + 2 * P.pad;
        // a remainder of one or two frames (the 49th of the standard window) would cost a whole eight-frame pass: it gets a tail pass
        // with 32 lanes per frame (kws_mfcc_kernel's layout)
        const int n_tail = (nfr >= KWS_M8_CHUNK && (nfr & 7) != 0 && (nfr & 7) <= 2) ? (nfr & 7) : 0;
        const int n_pass = n_tail ? nfr / KWS_M8_CHUNK : (nfr + KWS_M8_CHUNK - 1) / KWS_M8_CHUNK;
        const int *const pad_map = R.pad_maps + (size_t)nfr * R.map_stride;
        // per-lane constants of the spectral phase, re-derived per clip from a lane index the compiler cannot see through: hoisted out
        // of the clip loop they would stay live through cmvnw (three dozen registers) for ~100 L2-resident loads per clip
        int lane_c = lane;
        asm volatile("" : "+v"(lane_c));
        const int fl = lane_c & 7, fg = lane_c >> 3;
        // blocks fl (output positions 8 fl ..) and fl + 8: block j = 4 i1 + i2 reads input points i1 + 4 i2 + 16 i3 + 64 i4
        const int nbA = (fl >> 2) + 4 * (fl & 3);
        const cf a1 = to_cf(P.tw[16]), a2 = to_cf(P.tw[32]), a3 = to_cf(P.tw[48]);
        const cf b1 = to_cf(P.tw[4 * fl]), b2 = to_cf(P.tw[8 * fl]), b3 = to_cf(P.tw[12 * fl]);
        cf c1[4], c2[4], c3[4];
#pragma unroll
        for (int a = 0; a < 4; ++a) { c1[a] = to_cf(P.tw[fl + 8 * a]); c2[a] = to_cf(P.tw[2 * (fl + 8 * a)]); c3[a] = to_cf(P.tw[3 * (fl + 8 * a)]); }
        // split twiddles of this lane's eight bin pairs (k, 128 - k), k = fl + 8 a + 32 b for b < 2; lane 0's first pair is (64, 64)
        cf stw[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const int k = fl + 8 * (q & 3) + 32 * (q >> 2);
            stw[q] = to_cf(P.stw[(k == 0 ? KWS_NC / 2 : k) - 1]);
        }
        const int xwr = fg * XS + 18 * fl;                              // exchange buffer: position p of a frame at 2 p + 2 (p / 8)
        const int xrd = fg * XS + 2 * fl;
        const int partner = (lane_c & ~7) | ((8 - fl) & 7);
        const int half = lane_c >> 5, t = lane_c & 31;
        const int16_t *xbase = rc.x;
        // x[-1] of the window's first sample: the last sample of THIS clip (processing.hpp:68, 104-106)
        const float wrap_prev = (float)xbase[n_samples - 1] * (1.0f / 32768.0f);
        // a point's four samples x[2n - 2 .. 2n + 1] of frame f, requested one pass ahead
        auto fetch = [&](int q, fast_i2 (&raw)[2][8]) {
            const int f = min(KWS_M8_CHUNK * q + fg, nfr - 1);
            const int16_t *xf = xbase + (f * frame_stride + 2 * nbA - 2);
#pragma unroll
            for (int blk = 0; blk < 2; ++blk)
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    const int16_t *src = xf + (4 * blk + 32 * (i >> 1) + 128 * (i & 1));
                    if (blk == 0 && i == 0) src = src < xbase ? xbase : src;
                    raw[blk][i] = *(const fast_i2 *)src;
                }
        };
        // the frames of the pass after that: one 64-byte segment per lane, a pass before the real requests (see kws_fast_kernel)
        auto touch = [&](int q) {
            const int f = min(KWS_M8_CHUNK * q + fg, nfr - 1);
            return *(const int *)(xbase + (f * frame_stride + 32 * fl));
        };
        // ---- frame energy (feature.hpp:289-298): sequential fp32 sum over the 129 bins of a power row (numpy.hpp:88-94) ----------
        auto energy_of = [&](const float *pl, int f) {
            float e = 0.0f;
            float4 cur[8], nxt4[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) cur[u] = *(const float4 *)(pl + 4 * u);
#pragma unroll
            for (int k0 = 0; k0 < KWS_NBINS - 1; k0 += 32) {
                if (k0 + 32 < KWS_NBINS - 1) {
#pragma unroll
                    for (int u = 0; u < 8; ++u) nxt4[u] = *(const float4 *)(pl + k0 + 32 + 4 * u);
                }
#pragma unroll
                for (int u = 0; u < 8; ++u) { e += cur[u].x; e += cur[u].y; e += cur[u].z; e += cur[u].w; }
#pragma unroll
                for (int u = 0; u < 8; ++u) cur[u] = nxt4[u];
            }
            e += pl[KWS_NBINS - 1];
            if (e == 0.0f) e = FLT_EPSILON;                                           // feature.hpp:296-298
            sm.energy[f] = e;
        };
        // ---- mel filterbank for the frames of a pass: dot_by_row (numpy.hpp:183-211) as an ascending-bin gather, zero handling, log.
        //      pairs = pairs of frame slots a lane half walks (2: slots 4 h .. 4 h + 3 of an eight-frame pass; 1: the tail pass, slots 0, 1)
        auto mel_phase = [&](int fbase, int nfc, int pairs) {
            const float *p1 = pw + 4 * half * PS, *p2 = pw + fg * PS;
            float macc[5] = { 1.0f, 1.0f, 1.0f, 1.0f, 1.0f };
            {
                // filter lane & 31 for four of the pass's frame slots
                float w1[NZ];
                int fb1[NZ];
#pragma unroll
                for (int n = 0; n < NZ; ++n) { w1[n] = sm.tap_w[n * NF + t]; fb1[n] = sm.tap_b[n * NF + t]; }
#pragma unroll
                for (int s2 = 0; s2 < 4; s2 += 2) {
                    if (s2 >= 2 * pairs) break;
                    float xv[2][NZ];
#pragma unroll
                    for (int s = 0; s < 2; ++s)
#pragma unroll
                        for (int n = 0; n < NZ; ++n) xv[s][n] = p1[(s2 + s) * PS + fb1[n]];
#pragma unroll
                    for (int s = 0; s < 2; ++s) {
                        float acc = 0.0f;
#pragma unroll
                        for (int n = 0; n < NZ; ++n) {
                            const float prod = xv[s][n] * w1[n];
                            acc += prod;
                        }
                        macc[s2 + s] = acc;
                    }
                }
            }
            if constexpr (NF > 32) {
                // with 40 filters also filter 32 + lane & 7 for one slot
                float w2[NZ], xv2[NZ];
#pragma unroll
                for (int n = 0; n < NZ; ++n) { w2[n] = sm.tap_w[n * NF + 32 + fl]; xv2[n] = p2[sm.tap_b[n * NF + 32 + fl]]; }
                float acc = 0.0f;
#pragma unroll
                for (int n = 0; n < NZ; ++n) {
                    const float prod = xv2[n] * w2[n];
                    acc += prod;
                }
                macc[4] = acc;
            }
            auto put = [&](int slot, int j, float a) {
                if (a == 0.0f) a = FLT_EPSILON;                                       // functions.hpp:63-69
                sm.mel[(fbase + slot) * MELS + j] = fast_log(a);
            };
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                const int slot = 4 * half + s;
                if (s < 2 * pairs && slot < nfc && t < NF) put(slot, t, macc[s]);
            }
            if constexpr (NF > 32)
                if (fg < nfc && 32 + fl < NF) put(fg, 32 + fl, macc[4]);
        };

        fast_i2 nxt[2][8];
        fetch(0, nxt);
        asm volatile("" : : "v"(touched_next));
        int touched = touch(1);
        for (int q = 0; q < n_pass; ++q) {
            const int fbase = KWS_M8_CHUNK * q;
            const int f = fbase + fg;
            const bool live = f < nfr;
            cf u[4][4];                                                  // after the exchange: u[a][b] = position fl + 8 a + 32 b
            {
                cf z[2][8];
#pragma unroll
                for (int blk = 0; blk < 2; ++blk)
#pragma unroll
                    for (int i = 0; i < 8; ++i) z[blk][i] = exact_point(nxt[blk][i], pre_cof);
                if (f == 0 && fl == 0) {                                 // the clip's first sample: its predecessor wraps
                    const fast_i2 v = nxt[0][0];                         // (the request was clamped to the window's start: v.x = x[0], x[1])
                    const float lo = (float)(short)(v.x & 0xffff) * (1.0f / 32768.0f), hi = (float)(v.x >> 16) * (1.0f / 32768.0f);
                    const float pl = pre_cof * wrap_prev;
                    z[0][0].r = lo - pl;
                    const float ph_ = pre_cof * lo;
                    z[0][0].i = hi - ph_;
                }
                // unconditional (the frame index is clamped): a conditional request makes the compiler copy all sixteen register
                // pairs around the branch
                fetch(q + 1, nxt);
                asm volatile("" : : "v"(touched));
                touched = touch(q + 2);
                // kf_bfly2 (m = 1, twiddle 1) on the (i4 = 0, 1) pairs, then kf_bfly4 (m = 2) on the sums (k = 0) and the
                // differences (k = 1): outputs 8 j + k + 2 i
#pragma unroll
                for (int blk = 0; blk < 2; ++blk) {
                    cf sv[4], df[4];
#pragma unroll
                    for (int i = 0; i < 4; ++i) { sv[i] = cadd(z[blk][2 * i], z[blk][2 * i + 1]); df[i] = csub(z[blk][2 * i], z[blk][2 * i + 1]); }
                    bfly4_unit(sv[0], sv[1], sv[2], sv[3]);
                    bfly4(df[0], df[1], df[2], df[3], a1, a2, a3);
#pragma unroll
                    for (int i = 0; i < 4; ++i) { z[blk][2 * i] = sv[i]; z[blk][2 * i + 1] = df[i]; }
                }
                // the exchange, half a frame at a time (64 positions per frame fit the buffer): block fl feeds b = 0, 1
#pragma unroll
                for (int rnd = 0; rnd < 2; ++rnd) {
#pragma unroll
                    for (int r = 0; r < 8; ++r) *(float2 *)(xw + xwr + 2 * r) = make_float2(z[rnd][r].r, z[rnd][r].i);
                    WAVE_SYNC();
#pragma unroll
                    for (int b = 0; b < 2; ++b)
#pragma unroll
                        for (int a = 0; a < 4; ++a) {
                            const float2 v = *(const float2 *)(xw + xrd + 18 * a + 72 * b);
                            u[a][2 * rnd + b].r = v.x; u[a][2 * rnd + b].i = v.y;
                        }
                    WAVE_SYNC();
                }
            }
            // kf_bfly4 m = 8 (k = fl) inside every block of 32, then m = 32 (k = fl + 8 a) across them
#pragma unroll
            for (int b = 0; b < 4; ++b) bfly4(u[0][b], u[1][b], u[2][b], u[3][b], b1, b2, b3);
#pragma unroll
            for (int a = 0; a < 4; ++a) bfly4(u[a][0], u[a][1], u[a][2], u[a][3], c1[a], c2[a], c3[a]);
            // ---- kiss_fftr split (kiss_fftr.cpp:84-119) and the power spectrum (bin_power).  Bin pair (k, 128 - k) needs positions
            //      k and 128 - k: the second lives in lane (8 - fl) % 8 at (3 - a, 3 - b) -- in lane 0 itself, one position further --
            //      so the lanes swap their upper halves.
            {
                float *prw = pw + fg * PS;                           // (a row of a dead frame slot is written too, never used)
                const bool lane0 = fl == 0;
#pragma unroll
                for (int qq = 0; qq < 8; ++qq) {
                    const int a = qq & 3, b = qq >> 2;
                    cf other;
                    other.r = __int_as_float(__builtin_amdgcn_ds_bpermute(partner << 2, __float_as_int(u[3 - a][3 - b].r)));
                    other.i = __int_as_float(__builtin_amdgcn_ds_bpermute(partner << 2, __float_as_int(u[3 - a][3 - b].i)));
                    cf fpk = u[a][b];
                    int k = fl + 8 * a + 32 * b;
                    {
                        // lane 0: 128 - k = 8 (16 - a - 4 b) is position index 16 - qq of the lane itself; its pair 0 is (64, 64)
                        const int o = qq == 0 ? 8 : 16 - qq;
                        other.r = lane0 ? u[o & 3][o >> 2].r : other.r;
                        other.i = lane0 ? u[o & 3][o >> 2].i : other.i;
                        if (qq == 0) { fpk.r = lane0 ? u[0][2].r : fpk.r; fpk.i = lane0 ? u[0][2].i : fpk.i; k = lane0 ? KWS_NC / 2 : k; }
                    }
                    cf fpnk; fpnk.r = other.r; fpnk.i = -other.i;
                    const cf f1k = cadd(fpk, fpnk), f2k = csub(fpk, fpnk);
                    const cf twv = cmul(f2k, stw[qq]);
                    cf lo, hi;
                    lo.r = (f1k.r + twv.r) * 0.5f;                   // HALF_OF
                    lo.i = (f1k.i + twv.i) * 0.5f;
                    hi.r = (f1k.r - twv.r) * 0.5f;
                    hi.i = (twv.i - f1k.i) * 0.5f;
                    // bin 64 is written twice by the reference and the second store (the "ncfft - k" one) wins: same order here
                    prw[k] = bin_power(lo, inv_fft);
                    prw[KWS_NC - k] = bin_power(hi, inv_fft);
                }
                if (lane0) {                                         // tmp[0]: DC and Nyquist bins (kiss_fftr.cpp:84-96)
                    cf dc, ny;
                    dc.r = u[0][0].r + u[0][0].i; dc.i = 0.0f;
                    ny.r = u[0][0].r - u[0][0].i; ny.i = 0.0f;
                    prw[0] = bin_power(dc, inv_fft);
                    prw[KWS_NC] = bin_power(ny, inv_fft);
                }
            }
            WAVE_SYNC();
            if (fl == 0 && live) energy_of(pw + fg * PS, f);
            mel_phase(fbase, min(KWS_M8_CHUNK, nfr - fbase), 2);
            WAVE_SYNC();                                             // the next pass's exchange overwrites the power rows
        }

        if (n_tail) {
            // ---- tail pass: frame 8 n_pass + h on lane half h, a lane transforms four of its frame's 128 points per stage (kws_mfcc_kernel's
            //      butterflies): kf_bfly2 (m = 1) fused with kf_bfly4 (m = 2), then kf_bfly4 m = 8 and m = 32, each through an in-place,
            //      padded buffer behind the two power rows it feeds
            const int ft = KWS_M8_CHUNK * n_pass + half;
            const bool live_t = ft < nfr;
            const int s0 = min(ft, nfr - 1) * frame_stride + 8 * t;
            const int4 rawv = *(const int4 *)(xbase + s0);
            // (s0 = 0 needs a window of one frame: no tail pass then)
            const float rawp = s0 == 0 ? wrap_prev : (float)xbase[s0 - 1] * (1.0f / 32768.0f);
            const int k01 = t & 1, g01 = t >> 1, n0 = (g01 >> 2) + 4 * (g01 & 3), K2 = t & 7, G2 = t >> 3;
            const cf ta1 = to_cf(P.tw[16 * k01]), ta2 = to_cf(P.tw[32 * k01]), ta3 = to_cf(P.tw[48 * k01]);
            const cf tb1 = to_cf(P.tw[4 * K2]), tb2 = to_cf(P.tw[8 * K2]), tb3 = to_cf(P.tw[12 * K2]);
            const cf tc1 = to_cf(P.tw[t]), tc2 = to_cf(P.tw[2 * t]), tc3 = to_cf(P.tw[3 * t]);
            float *zb = sm.r1 + 2 * PS + half * KWS_ZF;
            {
                float y[8];
                float prev = rawp;
                const int w[4] = { rawv.x, rawv.y, rawv.z, rawv.w };
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const float lo = (float)(short)(w[i] & 0xffff) * (1.0f / 32768.0f);   // numpy::int16_to_float
                    const float hi = (float)(short)(w[i] >> 16) * (1.0f / 32768.0f);
                    const float pl = pre_cof * prev;
                    y[2 * i] = lo - pl;
                    const float ph_ = pre_cof * lo;
                    y[2 * i + 1] = hi - ph_;
                    prev = hi;
                }
                *(float4 *)(zb + 2 * zi(4 * t)) = make_float4(y[0], y[1], y[2], y[3]);
                *(float4 *)(zb + 2 * zi(4 * t) + 4) = make_float4(y[4], y[5], y[6], y[7]);
            }
            WAVE_SYNC();
            cf v[4];
            {
                cf la[4], lb[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) { la[i] = ld_cf(zb, n0 + 16 * i); lb[i] = ld_cf(zb, n0 + 16 * i + 64); }
#pragma unroll
                for (int i = 0; i < 4; ++i) v[i] = k01 ? csub(la[i], lb[i]) : cadd(la[i], lb[i]);
            }
            bfly4(v[0], v[1], v[2], v[3], ta1, ta2, ta3);
            WAVE_SYNC();                                              // every lane has read its inputs
#pragma unroll
            for (int i = 0; i < 4; ++i) st_cf(zb, 8 * g01 + k01 + 2 * i, v[i]);
            WAVE_SYNC();
#pragma unroll
            for (int i = 0; i < 4; ++i) v[i] = ld_cf(zb, 32 * G2 + K2 + 8 * i);
            bfly4(v[0], v[1], v[2], v[3], tb1, tb2, tb3);
#pragma unroll
            for (int i = 0; i < 4; ++i) st_cf(zb, 32 * G2 + K2 + 8 * i, v[i]);
            WAVE_SYNC();
#pragma unroll
            for (int i = 0; i < 4; ++i) v[i] = ld_cf(zb, t + 32 * i);
            bfly4(v[0], v[1], v[2], v[3], tc1, tc2, tc3);
#pragma unroll
            for (int i = 0; i < 4; ++i) st_cf(zb, t + 32 * i, v[i]);
            WAVE_SYNC();
            {
                const cf st1 = to_cf(P.stw[t]), st2 = to_cf(P.stw[t + 32]);
                cf fpk[2], fq[2];
#pragma unroll
                for (int rep = 0; rep < 2; ++rep) {
                    const int k = t + 1 + 32 * rep;
                    fpk[rep] = ld_cf(zb, k);
                    fq[rep] = ld_cf(zb, KWS_NC - k);
                }
                const float2 d0 = *(const float2 *)zb;                // tmp[0]: DC and Nyquist bins (kiss_fftr.cpp:84-96)
                float *prw = pw + half * PS;
#pragma unroll
                for (int rep = 0; rep < 2; ++rep) {
                    const int k = t + 1 + 32 * rep;
                    const cf stw_ = rep ? st2 : st1;
                    cf fpnk; fpnk.r = fq[rep].r; fpnk.i = -fq[rep].i;
                    const cf f1k = cadd(fpk[rep], fpnk), f2k = csub(fpk[rep], fpnk);
                    const cf twv = cmul(f2k, stw_);
                    cf lo, hi;
                    lo.r = (f1k.r + twv.r) * 0.5f;
                    lo.i = (f1k.i + twv.i) * 0.5f;
                    hi.r = (f1k.r - twv.r) * 0.5f;
                    hi.i = (twv.i - f1k.i) * 0.5f;
                    const float plo = bin_power(lo, inv_fft), phi = bin_power(hi, inv_fft);
                    if (k != KWS_NC / 2) prw[k] = plo;                // bin 64 is written twice by the reference: the second store wins
                    prw[KWS_NC - k] = phi;
                }
                if (t == 0) {
                    cf dc, ny;
                    dc.r = d0.x + d0.y; dc.i = 0.0f;
                    ny.r = d0.x - d0.y; ny.i = 0.0f;
                    prw[0] = bin_power(dc, inv_fft);
                    prw[KWS_NC] = bin_power(ny, inv_fft);
                }
            }
            WAVE_SYNC();
            if (t == 0 && live_t) energy_of(pw + half * PS, ft);
            mel_phase(KWS_M8_CHUNK * n_pass, n_tail, 1);
            WAVE_SYNC();
        }

        // ---- DCT-II via NF-point kiss_fftr, one frame per lane (numpy.hpp:378-401, fast-dct-fft.cpp:37-80): the cepstra of a frame
        //      replace its log-mel row in place (row stride MELS); cmvnw's pad map moves into the dead spectral buffers
        // (lane-derived constants of the DCT and of cmvnw are re-derived per clip as well: hoisted out of the clip loop they are spilled)
        int lane_d = lane;
        asm volatile("" : "+v"(lane_d));
        for (int i = lane_d; i < prow; i += KWS_WAVE) sm_map[i] = pad_map[i];
        // the wave's next clip: its first pass's samples are warmed in the cache while cmvnw runs
        if (clip + (int)gridDim.x < n_clips) {
            const KwsRaggedClip rn = R.clips[clip + gridDim.x];            // the next clip's own base and frame count
            touched_next = *(const int *)(rn.x + (min(fg, rn.frames - 1) * frame_stride + 32 * fl));
        }
        if (lane_d < nfr) {
            float v[NF];
            float *mrow = sm.mel + lane_d * MELS;
#pragma unroll
            for (int i = 0; i < NF; ++i) v[i] = mrow[i];
            float *orow = mrow;
            typedef KwsDctTab<NF> T;
            auto put = [&](int i, cf R) {
                float a = R.r * T::cs[i];
                float b = R.i * T::sn[i];
                float d = (a + b) * 2.0f;
                d = d * (i == 0 ? T::s0 : T::s1);
                orow[i] = d;
            };
            // coefficients above N/2 are never written by the transform: they keep the log-mel input (x2, scaled)
            if constexpr (NF == 32) {
                cf R[NCEPT];
                dct_spectrum<NF>(v, [&](int i, cf r) { R[i] = r; });
#pragma unroll
                for (int i = 0; i < NCEPT; ++i) put(i, R[i]);
#pragma unroll
                for (int i = NCEPT; i < NF; ++i)
                    if (i < ncep) orow[i] = (v[i] * 2.0f) * T::s1;
            } else {
                for (int i = NCEPT; i < ncep; ++i) orow[i] = (mrow[i] * 2.0f) * T::s1;
                dct_spectrum<NF>(v, put);
            }
            orow[0] = fast_log(sm.energy[lane_d]);                                       // feature.hpp:425-429
        }
        WAVE_SYNC();

        // ---- cmvnw (processing.hpp:326-389) + input quantisation ---------------------------------------------
        {
            float *fout = features ? features + (size_t)clip * out_stride : nullptr;
            int8_t *qclip = q_out ? q_out + (size_t)clip * out_stride : nullptr;
            // the rows that do not fit: the zeros of the reference's calloc'd matrix and their quantisation
            const int8_t qz = quantize_feature(0.0f, in_scale, in_zp);
            for (int i = nfr * ncep + lane_d; i < out_stride; i += KWS_WAVE) {
                if (fout) fout[i] = 0.0f;
                if (qclip) qclip[i] = qz;
            }
            auto emit = [&](int row, int c, float o) {
                const int idx = row * ncep + c;
                if (fout) fout[idx] = o;                      // optional output (extract_mfcc_features' matrix)
                if (qclip) qclip[idx] = quantize_feature(o, in_scale, in_zp);
            };
            if constexpr (WIDE) cmvn_columns<17, 20>(sm.mel, MELS, sm_map, offt, lane_d, nfr, ncep, prow, P.win_size, emit);
            else cmvn_columns<13, 16>(sm.mel, MELS, sm_map, offt, lane_d, nfr, ncep, prow, P.win_size, emit);
        }
        WAVE_SYNC();
    }
    asm volatile("" : : "v"(touched_next));
}

// One workgroup per slot: the clip's samples, two bytes at a time (the source has any alignment), zeros up to the slot's end.
__global__ __launch_bounds__(256) void kws_ragged_stage_kernel(const KwsRaggedClip *__restrict__ list, int n, int16_t *__restrict__ dst, int slot_stride,
                                                               float *__restrict__ wrap)
{
    for (int j = blockIdx.x; j < n; j += gridDim.x) {
        const KwsRaggedClip d = list[j];
        int16_t *out = dst + (size_t)j * slot_stride;
        for (int i = threadIdx.x; i < slot_stride; i += blockDim.x) out[i] = i < d.length ? d.x[i] : (int16_t)0;
        if (wrap && threadIdx.x == 0) wrap[j] = (float)d.x[d.length - 1] * (1.0f / 32768.0f);      // numpy::int16_to_float
    }
}

__global__ __launch_bounds__(256) void kws_ragged_scatter_kernel(const float *__restrict__ packed, const KwsRaggedClip *__restrict__ list, int n, int n_valid,
                                                                 int row_len, float *__restrict__ features, int8_t *__restrict__ q_out, float in_scale, int in_zp)
{
    for (int j = blockIdx.x; j < n; j += gridDim.x) {
        const size_t row = (size_t)list[j].frames * row_len;
        const float *src = packed + (size_t)j * n_valid;
        for (int i = threadIdx.x; i < row_len; i += blockDim.x) {
            const float v = i < n_valid ? src[i] : 0.0f;
            if (features) features[row + i] = v;
            if (q_out) q_out[row + i] = quantize_feature(v, in_scale, in_zp);
        }
    }
}

struct RaggedLaunchArgs {
    dim3 grid;
    hipStream_t stream;
    KwsDspPlan P;
    KwsRaggedArgs R;
    int n_clips;
    float *features;
    int8_t *q_out;
    float in_scale;
    int in_zp, out_stride;
};
template <int NZ, int NF, bool WIDE, int OCC>
static void ragged_launch(const RaggedLaunchArgs &a)
{
    hipLaunchKernelGGL((kws_mfcc8_ragged_kernel<NZ, NF, WIDE, OCC>), a.grid, dim3(KWS_WAVE), 0, a.stream, a.P, a.R, a.n_clips, a.features, a.q_out, a.in_scale,
                       a.in_zp, a.out_stride);
}
// the rows of kws_mfcc.hip's table that launch kws_mfcc8_kernel with cmvnw, in its order: the first whose limits cover the plan
struct RaggedVariant {
    int n_filters, max_nz, min_cepstra;
    void (*launch)(const RaggedLaunchArgs &);
};
static const RaggedVariant *ragged_variant(const KwsDspPlan &P)
{
    static const RaggedVariant table[] = {
        { 40, 8, 17, ragged_launch<8, 40, true, 2> },
        { 40, 8, 0, ragged_launch<8, 40, false, 2> },
        { 40, KWS_MAXNZ, 0, ragged_launch<KWS_MAXNZ, 40, false, 2> },
        { 32, 4, 0, ragged_launch<4, 32, false, 2> },
        { 32, KWS_MAXNZ, 0, ragged_launch<KWS_MAXNZ, 32, false, 2> },
    };
    if (P.generic || P.fft_len != KWS_FFT || P.n_frames + 2 * P.pad > KWS_MAXPROW) return nullptr;
    for (const RaggedVariant &v : table)
        if (v.n_filters == P.n_filters && P.max_nz <= v.max_nz && P.n_cepstral >= v.min_cepstra) return &v;
    return nullptr;
}
bool kws_mfcc_ragged_serves(const KwsDspPlan &P) { return ragged_variant(P) != nullptr; }

int kws_launch_mfcc_ragged(const KwsDspPlan &P, const KwsRaggedArgs &R, int n_clips, float *features, int8_t *q_out, float in_scale, int in_zp,
                           int out_stride, int grid_cap, hipStream_t stream)
{
    (void)hipGetLastError();      // the status returned below is this launch's, not a stale error of an earlier call
    if (n_clips <= 0) return 0;
    const RaggedVariant *v = ragged_variant(P);
    if (!v) return (int)hipErrorInvalidValue;
    RaggedLaunchArgs a = { dim3(n_clips < grid_cap ? n_clips : grid_cap), stream, P, R, n_clips, features, q_out, in_scale, in_zp, out_stride };
    v->launch(a);
    return (int)hipGetLastError();
}

int kws_launch_ragged_stage(const KwsRaggedClip *list, int n, int16_t *dst, int slot_stride, float *wrap, hipStream_t stream)
{
    (void)hipGetLastError();
    if (n <= 0) return 0;
    hipLaunchKernelGGL(kws_ragged_stage_kernel, dim3(n < 65536 ? n : 65536), dim3(256), 0, stream, list, n, dst, slot_stride, wrap);
    return (int)hipGetLastError();
}

int kws_launch_ragged_scatter(const float *packed, const KwsRaggedClip *list, int n, int n_valid, int row_len, float *features, int8_t *q_out,
                              float in_scale, int in_zp, hipStream_t stream)
{
    (void)hipGetLastError();
    if (n <= 0) return 0;
    hipLaunchKernelGGL(kws_ragged_scatter_kernel, dim3(n < 65536 ? n : 65536), dim3(256), 0, stream, packed, list, n, n_valid, row_len, features, q_out, in_scale,
                       in_zp);
    return (int)hipGetLastError();
}
