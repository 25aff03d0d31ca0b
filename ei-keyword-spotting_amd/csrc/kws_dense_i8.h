// kws_dense_i8.h -- kws_dense_i8_kernel: the dense stack of an int8 graph (1 .. 4 FULLY_CONNECTED, integer_ops/fully_connected.h:23-63, then
// SOFTMAX) for tiles of 16 clips on v_mfma_i32_16x16x64_i8.  Part of kws_nn_int8.hip (included there).
//
// A dense layer over a batch is [clips x K] x [K x units] with the same weights for every clip, so a wave owns a TILE of 16 clips (a workgroup
// 16 x KWS_DENSE_WAVES) and walks the whole chain for it: A = 16 clips x 64 inputs (layer 0: straight from the int8 input tensor or the trunk's
// hand-off in HBM, every byte read once; later layers: the previous layer's output in the wave's LDS buffer), B = 16 units x 64 inputs as
// per-lane fragments the host laid out once (KwsDenseLayer::wfrag; staged in LDS where the layer fits KWS_DENSE_LDS_W, read from L2 as 1 KB
// rows otherwise).  A and B use the same slot -> k map (lane l: row l & 15, inputs 64 s + 16 (l >> 4) .. + 15), so the instruction's internal
// order of k is irrelevant; int32 accumulation is exact.  The zero points stay outside the contraction:
//   sum (x + in_off)(w + w_off) = sum x w + w_off sum x + [in_off sum w + K in_off w_off]      (the bracket: bias_eff, host)
// K is padded to 64 with zero WEIGHTS (and zero activations, so that sum x is that of the real inputs).  The epilogue is op_fc's:
// MultiplyByQuantizedMultiplier, output zero point, activation clamp.
#pragma once

constexpr int KWS_DENSE_WAVES = 4;
constexpr int KWS_DENSE_NT = 8;          // unit tiles per pass over the inputs (32 accumulator registers)

__host__ __device__ inline size_t kws_dense_i8_smem_bytes(const KwsDensePlan &D)
{
    // fragments | softmax tables | per wave: sum x [16], clip [16], two activation buffers of 16 rows
    return (size_t)D.lds_w_bytes + 256 * 4 + 256 + (size_t)KWS_DENSE_WAVES * (128 + 2 * 16 * (size_t)D.act_stride);
}

// One layer for the wave's 16 clips.  FIRST: src is global memory, row r at src + row_off[r] (row_off is per lane: lane & 15's row), L.k bytes;
// else src is the wave's LDS buffer with rows of `stride` bytes, zero beyond L.k up to L.kpad.
template <bool FIRST>
__device__ __forceinline__ void dense_i8_layer(const KwsDenseLayer &L, const int8_t *__restrict__ gsrc, const int8_t *lsrc, int8_t *dst, int stride,
                                               const unsigned char *lds_w, int *xsum, const int *clipv, int n_valid, int lane, bool last,
                                               const KwsDensePlan &D, const NnTaps &taps, int tap_off)
{
    const int r = lane & 15, g = lane >> 4;
    const int ks = L.kpad >> 6, nt = L.upad >> 4;
    const bool need_sum = L.w_off != 0;
    for (int p0 = 0; p0 < nt; p0 += KWS_DENSE_NT) {
        v4i acc[KWS_DENSE_NT];
#pragma unroll
        for (int j = 0; j < KWS_DENSE_NT; ++j) acc[j] = (v4i){ 0, 0, 0, 0 };
        int xs = 0;
        for (int s = 0; s < ks; ++s) {
            const int k0 = 64 * s + 16 * g;
            v4i a;
            if constexpr (FIRST) {
                if (k0 + 16 <= L.k) {
                    __builtin_memcpy(&a, gsrc + k0, 16);                     // rows of K bytes: no alignment to rely on
                } else {
                    // the row's tail: bytes past K read as zero (and never past the buffer)
                    int wv[4] = { 0, 0, 0, 0 };
                    for (int j = 0; j < 16; ++j)
                        if (k0 + j < L.k) wv[j >> 2] |= (int)((unsigned)(unsigned char)gsrc[k0 + j] << (8 * (j & 3)));
                    a = (v4i){ wv[0], wv[1], wv[2], wv[3] };
                }
            } else {
                a = *(const v4i *)(lsrc + r * stride + k0);
            }
            if (need_sum && p0 == 0) {
                xs = __builtin_amdgcn_sdot4(a.x, 0x01010101, xs, false);
                xs = __builtin_amdgcn_sdot4(a.y, 0x01010101, xs, false);
                xs = __builtin_amdgcn_sdot4(a.z, 0x01010101, xs, false);
                xs = __builtin_amdgcn_sdot4(a.w, 0x01010101, xs, false);
            }
#pragma unroll
            for (int j = 0; j < KWS_DENSE_NT; ++j) {
                if (p0 + j < nt) {
                    const size_t fo = ((size_t)(p0 + j) * ks + s) * 1024 + (size_t)lane * 16;
                    v4i b;
                    if (L.lds_off >= 0) b = *(const v4i *)(lds_w + L.lds_off + fo);
                    else b = *(const v4i *)(L.wfrag + fo);
                    acc[j] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a, b, acc[j], 0, 0, 0);
                }
            }
        }
        if (p0 == 0) {
            // sum x of clip r: the four k-groups' partial sums (lanes r, r + 16, r + 32, r + 48)
            xs += __shfl_xor(xs, 16);
            xs += __shfl_xor(xs, 32);
            if (lane < 16) xsum[lane] = need_sum ? xs : 0;
            WAVE_SYNC();
        }
        // accumulator register i of a 16 x 16 tile holds row (clip) 4 (lane >> 4) + i, column (unit) lane & 15
#pragma unroll
        for (int j = 0; j < KWS_DENSE_NT; ++j) {
            if (p0 + j < nt) {
                const int col = 16 * (p0 + j) + r;
                const int be = L.bias_eff[col];                              // [upad]
                const bool col_ok = col < L.units;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int row = 4 * g + i;
                    int v = acc[j][i] + L.w_off * xsum[row] + be;
                    v = mbqm(v, L.mult, L.shift) + L.out_zp;
                    v = min(max(v, L.act_min), L.act_max);
                    dst[row * stride + col] = col_ok ? (int8_t)v : (int8_t)0;
                    if (col_ok && row < n_valid) {
                        if (last) { if (taps.fc) taps.fc[(size_t)clipv[row] * L.units + col] = (int8_t)v; }
                        else if (taps.pooled) taps.pooled[(size_t)clipv[row] * taps.pooled_stride + tap_off + col] = (int8_t)v;
                    }
                }
            }
        }
    }
    // the next layer's K padding: zero activations from upad up to its 64
    const int kn = (L.units + 63) & ~63, npad = kn - L.upad;
    for (int i = lane; i < 16 * npad; i += 64) {
        const int row = i / npad, c = i - row * npad;
        dst[row * stride + L.upad + c] = 0;
    }
    WAVE_SYNC();
}

// x: by_clip = 1: the int8 input tensor [n_clips][K] (row = clip index); 0: the trunk's hand-off [ci - ci0][K].  List entries ci0 .. ci1 - 1
// (of the selection taps.sel, or clips themselves) are served.
__global__ __launch_bounds__(KWS_WAVE * KWS_DENSE_WAVES) void kws_dense_i8_kernel(KwsDensePlan D, const int8_t *__restrict__ x, int by_clip, int ci0,
                                                                                 int ci1, int n_clips, float *__restrict__ scores, NnTaps taps)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int n_end = min(sel_count(taps.sel, n_clips), ci1);
    const int n_tiles = (n_end - ci0 + 15) >> 4;
    if ((int)blockIdx.x * KWS_DENSE_WAVES >= n_tiles) return;          // (an empty re-run list of a KWS_MODE_FAST call: before anything is staged)
    unsigned char *lds_w = smem_raw;
    for (int i = threadIdx.x * 16; i < D.lds_w_bytes; i += blockDim.x * 16) {
        // which layer's fragments does byte i belong to?  (layers are laid out in order, 1 KB granules)
        const unsigned char *src = nullptr;
#pragma unroll
        for (int l = 0; l < KWS_DENSE_MAX; ++l)
            if (l < D.n_layers && D.l[l].lds_off >= 0 && i >= D.l[l].lds_off && i < D.l[l].lds_off + D.l[l].upad * D.l[l].kpad)
                src = (const unsigned char *)D.l[l].wfrag + (i - D.l[l].lds_off);
        if (src) *(v4i *)(lds_w + i) = *(const v4i *)src;
    }
    int *se = (int *)(smem_raw + D.lds_w_bytes);
    uint8_t *sv = (uint8_t *)(se + 256);
    for (int i = threadIdx.x; i < 256; i += blockDim.x) { se[i] = D.sm_exp[i]; sv[i] = D.sm_valid[i]; }
    const NnHeadTab H = { nullptr, nullptr, se, sv };
    const int stride = D.act_stride;
    unsigned char *wbase = smem_raw + D.lds_w_bytes + 256 * 4 + 256 + (size_t)wave * (128 + 2 * 16 * (size_t)stride);
    int *xsum = (int *)wbase, *clipv = xsum + 16;
    int8_t *bufA = (int8_t *)(wbase + 128), *bufB = bufA + 16 * stride;
    __syncthreads();

    for (int t = blockIdx.x * KWS_DENSE_WAVES + wave; t < n_tiles; t += gridDim.x * KWS_DENSE_WAVES) {
        const int cb = ci0 + 16 * t, n_valid = min(16, n_end - cb);
        // rows past the batch repeat the last clip (computed, never stored)
        const int ci = min(cb + (lane & 15), n_end - 1);
        const int clip = sel_clip(taps.sel, ci);
        if (lane < 16) clipv[lane] = clip;
        const int8_t *row = x + (size_t)(by_clip ? clip : ci - ci0) * D.l[0].k;
        WAVE_SYNC();
        int tap_off = D.tap_off;
        dense_i8_layer<true>(D.l[0], row, nullptr, bufA, stride, lds_w, xsum, clipv, n_valid, lane, D.n_layers == 1, D, taps, tap_off);
        tap_off += D.l[0].units;
        int8_t *cur = bufA, *nxt = bufB;
#pragma unroll
        for (int l = 1; l < KWS_DENSE_MAX; ++l) {
            if (l < D.n_layers) {
                dense_i8_layer<false>(D.l[l], nullptr, cur, nxt, stride, lds_w, xsum, clipv, n_valid, lane, l + 1 == D.n_layers, D, taps, tap_off);
                tap_off += D.l[l].units;
                int8_t *tmp = cur; cur = nxt; nxt = tmp;
            }
        }
        // SOFTMAX (reference/softmax.h:66-144), clip by clip: lane = class
        for (int rr = 0; rr < n_valid; ++rr) {
            const bool on = lane < D.n_labels;
            const int logit = on ? (int)cur[rr * stride + lane] : 0;
            nn_softmax(D.n_labels, D.out_zp, D.out_scale, H, on, logit, lane, clipv[rr], scores, taps);
        }
    }
}
