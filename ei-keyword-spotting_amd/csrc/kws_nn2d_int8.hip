// kws_nn2d_int8.hip -- kws_nn2d_trunk_kernel: the CONV_2D [+ MAX_POOL_2D] blocks of an int8 2-D graph, in front of kws_dense_i8_kernel.
// Replays integer_ops/conv.h:64-116 and integer_ops/pooling.h:82-137 with both spatial axes live.
//
// One wave per clip, persistent workgroups.  Per workgroup, once: every block's weights ([out_c][kh][krow4]: a filter row's kw * in_c operands, zero
// padded to whole dot4 words) and requantisation constants in LDS.  Per wave: two ping-pong images.  An image is the block's NHWC input behind its SAME
// padding, every padding byte the input zero point -- (x + input_offset) * w = 0 there, so a padded tap adds what the reference's skipped tap adds: nothing.
// In NHWC the kw * in_c operands of one filter row of one output are CONTIGUOUS bytes of one image row, so a filter row is a run of v_dot4 words; the run
// starts at byte (ox * stride_w * in_c) of the row, which is 4-byte aligned only by luck: each operand word is assembled from two aligned LDS words with
// v_alignbyte (never an unaligned LDS access).  The zero weights behind a filter row multiply whatever follows it in the image (the next pixels, the next
// row, the 16 bytes behind the buffer): exact zeros, int32 sums are order-free.
// A lane owns one POOLED output (py, px, oc): it runs the convolution at every position of its pooling window that lies inside the conv output (SAME pooling
// takes the max over those only, pooling.h:103-119), keeps the largest raw accumulator and requantises once -- requantisation and the clamp are
// non-decreasing (the plan refuses what would break that: kws_nn_int8_dev.h), so max commutes with them.  Overlapping windows (stride < window) repeat
// convolutions; no third buffer is needed.  oc is the fastest item index: the lanes of a wave read few distinct image addresses (broadcasts) and write
// consecutive bytes.
#include "kws_device.h"
#include "kws_nn_int8_dev.h"
#include "kws_nn2d.h"

__global__ __launch_bounds__(KWS_WAVE * KWS_NN2D_WAVES_MAX) void kws_nn2d_trunk_kernel(KwsNn2dPlan N, const int8_t *__restrict__ q_in, int n_clips,
                                                                                      int8_t *__restrict__ handoff, int ci0, int ci1, NnTaps taps)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), n_waves = blockDim.x >> 6;

    // ---- shared: weights and requantisation constants of every block, in block order ---------------------------
    unsigned char *sp = smem_raw;
    int img_b[2] = { 0, 0 };                           // block b reads image b & 1: each is sized for its own blocks
    for (int b = 0; b < N.n_blocks; ++b) {
        const KwsConv2dBlock &k = N.blk[b];
        for (int i = threadIdx.x * 4; i < k.w_bytes; i += blockDim.x * 4) *(int *)(sp + i) = *(const int *)(k.w + i);
        sp += (k.w_bytes + 15) & ~15;
        for (int i = threadIdx.x; i < k.g.out_c; i += blockDim.x) ((int4 *)sp)[i] = make_int4(k.bias_eff[i], k.mult[i], k.shift[i], 0);
        sp += k.g.out_c * 16;
        img_b[b & 1] = max(img_b[b & 1], kws_nn2d_img_bytes(k.g, 1));
    }
    int8_t *const imgA = (int8_t *)(sp + wave * (img_b[0] + img_b[1]));
    int8_t *const imgB = imgA + img_b[0];
    __syncthreads();

    const int n_sel = min(sel_count(taps.sel, n_clips), ci1);
    for (int ci = ci0 + blockIdx.x * n_waves + wave; ci < n_sel; ci += gridDim.x * n_waves) {
        const int clip = sel_clip(taps.sel, ci);
        // ---- stage the int8 input tensor [in_h][in_w][in_c] behind its padding (= zero point) ----------------------
        {
            const KwsConv2dBlock &k = N.blk[0];
            const KwsConv2dGeom &g = k.g;
            const int zp4 = (int)((unsigned)(k.in_zp & 0xff) * 0x01010101u);
            for (int i = lane * 16; i < kws_nn2d_img_bytes(g, 1); i += 64 * 16) *(int4 *)(imgA + i) = make_int4(zp4, zp4, zp4, zp4);
            WAVE_SYNC();
            const int8_t *src = q_in + (size_t)clip * N.n_features;
            const int row = g.in_w * g.in_c;
            for (int i = lane; i < g.in_h * row; i += 64) {
                const int y = i / row, x = i - y * row;
                imgA[(y + g.pad_t) * g.img_pitch + g.pad_l * g.in_c + x] = src[i];
            }
            WAVE_SYNC();
        }
        int8_t *cur = imgA, *nxt = imgB;
        int pooled_off = 0;
        const unsigned char *bp = smem_raw;
        for (int b = 0; b < N.n_blocks; ++b) {
            const KwsConv2dBlock &k = N.blk[b];
            const KwsConv2dGeom &g = k.g;
            const int8_t *wb = (const int8_t *)bp;
            bp += (k.w_bytes + 15) & ~15;
            const int4 *rqt = (const int4 *)bp;
            bp += g.out_c * 16;
            const bool last = (b + 1 == N.n_blocks);
            // where pooled output (py, px, oc) goes: the next block's image behind its padding, or the hand-off row (flattened NHWC)
            int8_t *dbase;
            int dpitch;
            if (!last) {
                const KwsConv2dBlock &nk = N.blk[b + 1];
                const int zp4 = (int)((unsigned)(nk.in_zp & 0xff) * 0x01010101u);
                for (int i = lane * 16; i < kws_nn2d_img_bytes(nk.g, 1); i += 64 * 16) *(int4 *)(nxt + i) = make_int4(zp4, zp4, zp4, zp4);
                WAVE_SYNC();
                dbase = nxt + nk.g.pad_t * nk.g.img_pitch + nk.g.pad_l * g.out_c;
                dpitch = nk.g.img_pitch;
            } else {
                dbase = handoff + (size_t)(ci - ci0) * N.out_n;
                dpitch = g.pool_w * g.out_c;
            }
            int8_t *const tp = taps.pooled ? taps.pooled + (size_t)clip * taps.pooled_stride + pooled_off : nullptr;
            const int out_c = g.out_c, n_items = g.pool_h * g.pool_w * out_c;
            const int n4 = g.krow4 >> 2, xstep = g.sw * g.in_c, ystep = g.sh * g.img_pitch;
            for (int item = lane; item < n_items; item += 64) {
                const int pos = item / out_c, oc = item - pos * out_c;
                const int py = pos / g.pool_w, px = pos - py * g.pool_w;
                // the window's conv outputs (cy0 + wy, cx0 + wx), clipped to the conv output
                const int cy0 = py * g.psh - g.ppt, cx0 = px * g.psw - g.ppl;
                const int wy0 = max(0, -cy0), wy1 = min(g.ph, g.out_h - cy0), wx0 = max(0, -cx0), wx1 = min(g.pw, g.out_w - cx0);
                const int *wrow = (const int *)(wb + (size_t)oc * g.kh * g.krow4);
                int m = (int)0x80000000;
                for (int wy = wy0; wy < wy1; ++wy)
                    for (int wx = wx0; wx < wx1; ++wx) {
                        const int s0 = (cy0 + wy) * ystep + (cx0 + wx) * xstep;          // byte of the image the output's first operand sits at
                        const unsigned mis = (unsigned)s0 & 3u;                          // (the pitch is a multiple of 4: the same for every filter row)
                        const int *xr = (const int *)(cur + (s0 & ~3));
                        int acc = 0;
                        for (int fy = 0; fy < g.kh; ++fy) {
                            const int *wr = wrow + fy * n4;
                            unsigned lo = (unsigned)xr[0];
                            for (int j = 0; j < n4; ++j) {
                                const unsigned hi = (unsigned)xr[j + 1];
                                acc = __builtin_amdgcn_sdot4(wr[j], (int)__builtin_amdgcn_alignbyte(hi, lo, mis), acc, false);
                                lo = hi;
                            }
                            xr += g.img_pitch >> 2;
                        }
                        m = max(m, acc);
                    }
                const int r = nn_requant(m, nn_rq_of(rqt, oc), k.out_zp, k.act_min, k.act_max);
                dbase[py * dpitch + px * out_c + oc] = (int8_t)r;
                if (tp) tp[item] = (int8_t)r;
            }
            pooled_off += n_items;
            WAVE_SYNC();
            int8_t *tmp = cur; cur = nxt; nxt = tmp;
        }
    }
}

int kws_launch_nn2d_trunk(const KwsNn2dPlan &N, const int8_t *q_in, int n_clips, int8_t *handoff, int ci0, int ci1, int8_t *tap_pooled, int pooled_stride,
                          const int *sel, int n_cu, hipStream_t stream)
{
    const int nw = kws_nn2d_waves(N), n = ci1 - ci0;
    if (nw == 0) return (int)hipErrorInvalidValue;           // (kws_create refuses such a graph)
    if (n <= 0) return 0;
    const size_t smem = kws_nn2d_smem_bytes(N, nw);
    if (smem > 64 * 1024) {                    // opt in to more than the default 64 KB of dynamic LDS
        hipError_t e = hipFuncSetAttribute((const void *)kws_nn2d_trunk_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
        if (e != hipSuccess) return (int)e;
    }
    int grid = (n + nw - 1) / nw;
    if (grid > n_cu) grid = n_cu;              // one persistent workgroup per CU
    NnTaps taps = { tap_pooled, pooled_stride, nullptr, nullptr, nullptr, sel };
    hipLaunchKernelGGL(kws_nn2d_trunk_kernel, dim3(grid), dim3(KWS_WAVE * nw), smem, stream, N, q_in, n_clips, handoff, ci0, ci1, taps);
    return (int)hipGetLastError();
}
