// kws_nnres_int8.hip -- kws_nnres_trunk_kernel: the steps of an int8 residual graph or depthwise-separable 2-D graph -- CONV_2D,
// DEPTHWISE_CONV_2D and ADD(tensor, tensor), each [+ MAX_POOL_2D], over H x W x C images, H >= 1 -- in front of kws_dense_i8_kernel.  Replays
// integer_ops/conv.h:64-116, integer_ops/depthwise_conv.h:22-120, integer_ops/add.h and integer_ops/pooling.h:82-137.
//
// The execution model of kws_nn2d_trunk_kernel (kws_nn2d_int8.hip): one wave per clip, persistent workgroups; per workgroup, once, every step's constants
// in LDS -- a convolution's weights ([out_c][kh][krow4]) and requantisation constants, an ADD's two operand tables.  Per wave: KWS_RES_SLOTS image buffers.
// A tensor is stored ONCE, in the slot the plan's liveness analysis gave it, behind a margin that is the largest top / left padding any of its consumers
// needs and every padding byte the tensor's zero point; a consumer with less padding (a 1 x 1 shortcut next to a 9-tap main path, an ADD) starts reading
// further in: the plan hands each step the offset of the first element its output (0, 0) reads.  A step first fills its destination image with the
// output tensor's zero point, then writes its outputs inside the margin; the last step writes the hand-off row instead.
// Convolution: kws_nn2d_trunk_kernel's arithmetic -- a lane owns one pooled output (py, px, oc), a filter row is a run of v_dot4 over operand words
// assembled with v_alignbyte from aligned LDS words, the window's largest raw accumulator is requantised once (max commutes with the non-decreasing
// requantisation; the plan refuses what would break that).
// Depthwise convolution: output channel oc reads input channel oc / depth_multiplier alone; the filter stays in the tensor's own [kh][kw][out_c] order, so
// at one tap the lanes of a position read neighbouring weight bytes and (depth multiplier 1) neighbouring image bytes -- one byte per lane, no two lanes on
// different dwords of a bank before 64 bytes are covered.  The same bias folding (a padding byte is the zero point and adds 0), the same single
// requantisation of the window's largest accumulator; the clamp is the int8 range whatever the node's fused activation says (depthwise_conv.cc:618-620:
// the plan sets act_min / act_max so).
// ADD: o = clamp(MBQM(q1[a] + q2[b], mo, so) + z_out), q1 / q2 the operands' 256-entry tables (the host built them with the reference's arithmetic:
// (x - z) << 20 through the operand's multiplier).  ADD is not monotone in the pair, so a pool behind it takes the maximum of the RESULTS at the positions
// of its window.
#include "kws_device.h"
#include "kws_nn_int8_dev.h"
#include "kws_nnres.h"

__global__ __launch_bounds__(KWS_WAVE * KWS_NNRES_WAVES_MAX) void kws_nnres_trunk_kernel(KwsResPlan N, const int8_t *__restrict__ q_in, int n_clips,
                                                                                        int8_t *__restrict__ handoff, int ci0, int ci1, NnTaps taps)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), n_waves = blockDim.x >> 6;

    // ---- shared: the constants of every step, in step order --------------------------------------------------------
    unsigned char *sp = smem_raw;
    for (int s = 0; s < N.n_steps; ++s) {
        const KwsResStep &k = N.st[s];
        if (k.g.kind != KWS_RES_ADD) {
            for (int i = threadIdx.x * 4; i < k.w_bytes; i += blockDim.x * 4) *(int *)(sp + i) = *(const int *)(k.w + i);
            sp += (k.w_bytes + 15) & ~15;
            for (int i = threadIdx.x; i < k.g.out_c * 4; i += blockDim.x) ((int *)sp)[i] = k.rq[i];
            sp += k.g.out_c * 16;
        } else {
            for (int i = threadIdx.x; i < KWS_NNRES_ADD_TAB_BYTES / 4; i += blockDim.x) ((int *)sp)[i] = k.rq[i];
            sp += KWS_NNRES_ADD_TAB_BYTES;
        }
    }
    int8_t *const wbase = (int8_t *)sp + (size_t)wave * N.wave_bytes;      // this wave's slots
    __syncthreads();

    const int n_sel = min(sel_count(taps.sel, n_clips), ci1);
    for (int ci = ci0 + blockIdx.x * n_waves + wave; ci < n_sel; ci += gridDim.x * n_waves) {
        const int clip = sel_clip(taps.sel, ci);
        // ---- stage the int8 input tensor [in_h][in_row] behind its margin (= zero point) ---------------------------------
        {
            int8_t *img = wbase + N.in_base;
            const int zp4 = (int)((unsigned)(N.in_zp & 0xff) * 0x01010101u);
            for (int i = lane * 16; i < N.in_bytes; i += 64 * 16) *(int4 *)(img + i) = make_int4(zp4, zp4, zp4, zp4);
            WAVE_SYNC();
            const int8_t *src = q_in + (size_t)clip * N.n_features;
            for (int i = lane; i < N.in_h * N.in_row; i += 64) {
                const int y = i / N.in_row, x = i - y * N.in_row;
                img[N.in_off + y * N.in_pitch + x] = src[i];
            }
            WAVE_SYNC();
        }
        int pooled_off = 0;
        const unsigned char *bp = smem_raw;
        for (int s = 0; s < N.n_steps; ++s) {
            const KwsResStep &k = N.st[s];
            const KwsResGeom &g = k.g;
            // where pooled output (py, px, oc) goes: the tensor's image behind its margin, or the hand-off row (flattened NHWC)
            int8_t *dbase;
            if (g.d_base >= 0) {
                int8_t *img = wbase + g.d_base;
                const int zp4 = (int)((unsigned)(k.d_zp & 0xff) * 0x01010101u);
                for (int i = lane * 16; i < g.d_bytes; i += 64 * 16) *(int4 *)(img + i) = make_int4(zp4, zp4, zp4, zp4);
                WAVE_SYNC();
                dbase = img + g.d_off;
            } else dbase = handoff + (size_t)(ci - ci0) * N.out_n;
            const int dpitch = g.d_pitch;
            int8_t *const tp = taps.pooled ? taps.pooled + (size_t)clip * taps.pooled_stride + pooled_off : nullptr;
            const int out_c = g.out_c, n_items = g.pool_h * g.pool_w * out_c;
            if (g.kind == KWS_RES_CONV) {
                const int8_t *wb = (const int8_t *)bp;
                bp += (k.w_bytes + 15) & ~15;
                const int4 *rqt = (const int4 *)bp;
                bp += out_c * 16;
                const int8_t *cur = wbase + g.a_base;
                const int n4 = g.krow4 >> 2, xstep = g.sw * g.in_c, ystep = g.sh * g.a_pitch;
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
                            const int s0 = g.a_off + (cy0 + wy) * ystep + (cx0 + wx) * xstep;  // byte of the slot the output's first operand sits at
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
                                xr += g.a_pitch >> 2;
                            }
                            m = max(m, acc);
                        }
                    const int r = nn_requant(m, nn_rq_of(rqt, oc), k.out_zp, k.act_min, k.act_max);
                    dbase[py * dpitch + px * out_c + oc] = (int8_t)r;
                    if (tp) tp[item] = (int8_t)r;
                }
            } else if (g.kind == KWS_RES_DW) {
                const int8_t *wb = (const int8_t *)bp;
                bp += (k.w_bytes + 15) & ~15;
                const int4 *rqt = (const int4 *)bp;
                bp += out_c * 16;
                const int8_t *cur = wbase + g.a_base + g.a_off;
                const int in_c = g.in_c, xstep = g.sw * in_c, ystep = g.sh * g.a_pitch, wrow = g.kw * out_c;
                for (int item = lane; item < n_items; item += 64) {
                    const int pos = item / out_c, oc = item - pos * out_c;
                    const int py = pos / g.pool_w, px = pos - py * g.pool_w;
                    const int cy0 = py * g.psh - g.ppt, cx0 = px * g.psw - g.ppl;
                    const int wy0 = max(0, -cy0), wy1 = min(g.ph, g.out_h - cy0), wx0 = max(0, -cx0), wx1 = min(g.pw, g.out_w - cx0);
                    const int ic = g.dm == 1 ? oc : oc / g.dm;
                    int m = (int)0x80000000;
                    for (int wy = wy0; wy < wy1; ++wy)
                        for (int wx = wx0; wx < wx1; ++wx) {
                            const int8_t *xr = cur + (cy0 + wy) * ystep + (cx0 + wx) * xstep + ic;
                            const int8_t *wr = wb + oc;
                            int acc = 0;
                            for (int fy = 0; fy < g.kh; ++fy) {
                                for (int fx = 0; fx < g.kw; ++fx) acc += (int)wr[fx * out_c] * (int)xr[fx * in_c];
                                xr += g.a_pitch;
                                wr += wrow;
                            }
                            m = max(m, acc);
                        }
                    const int r = nn_requant(m, nn_rq_of(rqt, oc), k.out_zp, k.act_min, k.act_max);
                    dbase[py * dpitch + px * out_c + oc] = (int8_t)r;
                    if (tp) tp[item] = (int8_t)r;
                }
            } else {
                const int *t1 = (const int *)bp, *t2 = t1 + 256;
                bp += KWS_NNRES_ADD_TAB_BYTES;
                const int8_t *pa = wbase + g.a_base + g.a_off, *pb = wbase + g.b_base + g.b_off;
                for (int item = lane; item < n_items; item += 64) {
                    const int pos = item / out_c, oc = item - pos * out_c;
                    const int py = pos / g.pool_w, px = pos - py * g.pool_w;
                    const int cy0 = py * g.psh - g.ppt, cx0 = px * g.psw - g.ppl;
                    const int wy0 = max(0, -cy0), wy1 = min(g.ph, g.out_h - cy0), wx0 = max(0, -cx0), wx1 = min(g.pw, g.out_w - cx0);
                    int m = -128;
                    for (int wy = wy0; wy < wy1; ++wy)
                        for (int wx = wx0; wx < wx1; ++wx) {
                            const int y = cy0 + wy, e = (cx0 + wx) * out_c + oc;
                            const int q = t1[(int)pa[y * g.a_pitch + e] + 128] + t2[(int)pb[y * g.b_pitch + e] + 128];
                            const int o = mbqm(q, k.add_mult, k.add_shift) + k.out_zp;            // integer_ops/add.h:108-131
                            m = max(m, min(k.act_max, max(k.act_min, o)));
                        }
                    dbase[py * dpitch + px * out_c + oc] = (int8_t)m;
                    if (tp) tp[item] = (int8_t)m;
                }
            }
            pooled_off += n_items;
            WAVE_SYNC();
        }
    }
}

int kws_launch_nnres_trunk(const KwsResPlan &N, const int8_t *q_in, int n_clips, int8_t *handoff, int ci0, int ci1, int8_t *tap_pooled, int pooled_stride,
                           const int *sel, int n_cu, hipStream_t stream)
{
    const int nw = kws_nnres_waves(N), n = ci1 - ci0;
    if (nw == 0) return (int)hipErrorInvalidValue;           // (kws_create refuses such a graph)
    if (n <= 0) return 0;
    const size_t smem = kws_nnres_smem_bytes(N, nw);
    if (smem > 64 * 1024) {                    // opt in to more than the default 64 KB of dynamic LDS
        hipError_t e = hipFuncSetAttribute((const void *)kws_nnres_trunk_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
        if (e != hipSuccess) return (int)e;
    }
    int grid = (n + nw - 1) / nw;
    if (grid > n_cu) grid = n_cu;              // one persistent workgroup per CU
    NnTaps taps = { tap_pooled, pooled_stride, nullptr, nullptr, nullptr, sel };
    hipLaunchKernelGGL(kws_nnres_trunk_kernel, dim3(grid), dim3(KWS_WAVE * nw), smem, stream, N, q_in, n_clips, handoff, ci0, ci1, taps);
    return (int)hipGetLastError();
}
