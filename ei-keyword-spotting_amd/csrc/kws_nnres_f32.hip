// kws_nnres_f32.hip -- kws_nnres_f32_trunk_kernel: the steps of a float32 residual graph or depthwise-separable 2-D graph --
// CONV_2D, DEPTHWISE_CONV_2D and ADD(tensor, tensor), each [+ MAX_POOL_2D] -- in front of kws_dense_f32_kernel.  Replays reference/conv.h:28-99,
// reference/depthwiseconv_float.h:25-97, reference/add.h and reference/pooling.h:189-237 in the reference's own order.
//
// The execution model and the image layout of kws_nnres_trunk_kernel (kws_nnres_int8.hip): one wave per clip, persistent workgroups, every tensor once in
// the slot the plan gave it, behind the largest margin its consumers need; padding is +0.0f.  The convolution is kws_nn2d_f32_trunk_kernel's: every output
// is ONE chain -- total += input * filter over fy, then fx, then ic, product and sum rounded separately (the build has -ffp-contract=off and kws_device.h
// switches contraction off), then + bias, then the clamp; a padded tap adds 0 * w = +-0 to a chain that started at +0, which changes nothing for a FINITE w
// (the plan refuses a non-finite weight).  The filters of the steps the plan marks (w_lds) are staged once per workgroup in LDS; a float twin's filters can
// exceed the LDS, and the plan leaves the largest ones in HBM, where the lanes read them through the caches.
// Depthwise convolution: output channel oc is one chain over fy, then fx, of input channel oc / depth_multiplier times filter [fy][fx][oc] (the tensor's own
// [kh][kw][out_c] order, in LDS or HBM as a convolution's), then + bias (+ 0.0f where the node has none: the plan uploads zeros), then the fused
// activation's clamp, which the float op honours (depthwise_conv.cc:582-603).
// ADD: clamp(a + b), one rounded add; whatever the operands hold (+-0, subnormals, +-inf, NaN) meets the same instruction as in the reference.
// MAX_POOL_2D behind either: std::max over the window's in-image RESULTS in the reference's order (max = max < v ? v : max from lowest(): a NaN never wins),
// then the pool's own clamp.
#include <algorithm>

#include "kws_device.h"
#include "kws_nnres.h"

__device__ __forceinline__ float nnres_clamp(float x, float lo, float hi)   // ActivationFunctionWithMinMax: std::min(std::max(x, lo), hi)
{
    const float a = x < lo ? lo : x;
    return hi < a ? hi : a;
}

__global__ __launch_bounds__(KWS_WAVE * KWS_NNRES_WAVES_MAX) void kws_nnres_f32_trunk_kernel(KwsResPlanF32 N, const float *__restrict__ features, int n_clips,
                                                                                            float *__restrict__ handoff, int ci0, int ci1,
                                                                                            const int *__restrict__ sel)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), n_waves = blockDim.x >> 6;

    // ---- shared: the staged filters and every bias, in step order --------------------------------------------------
    float *sp = (float *)smem_raw;
    for (int s = 0; s < N.n_steps; ++s) {
        const KwsResStepF32 &k = N.st[s];
        if (k.g.kind == KWS_RES_ADD) continue;
        if (k.w_lds) {
            const int nw = k.g.out_c * k.g.kh * k.g.krow;
            for (int i = threadIdx.x; i < nw; i += blockDim.x) sp[i] = k.w[i];
            sp += (nw + 3) & ~3;
        }
        for (int i = threadIdx.x; i < k.g.out_c; i += blockDim.x) sp[i] = k.bias[i];
        sp += (k.g.out_c + 3) & ~3;
    }
    float *const wbase = (float *)((unsigned char *)sp + (size_t)wave * N.wave_bytes);      // this wave's slots
    __syncthreads();

    const int n_sel = min(sel_count(sel, n_clips), ci1);
    for (int ci = ci0 + blockIdx.x * n_waves + wave; ci < n_sel; ci += gridDim.x * n_waves) {
        const int clip = sel_clip(sel, ci);
        // ---- stage the feature matrix [in_h][in_row] behind its zero margin --------------------------------------------
        {
            float *img = wbase + N.in_base;
            for (int i = lane * 16; i < N.in_bytes; i += 64 * 16) *(float4 *)((unsigned char *)img + i) = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            WAVE_SYNC();
            const float *src = features + (size_t)clip * N.n_features;
            for (int i = lane; i < N.in_h * N.in_row; i += 64) {
                const int y = i / N.in_row, x = i - y * N.in_row;
                img[N.in_off + y * N.in_pitch + x] = src[i];
            }
            WAVE_SYNC();
        }
        const float *bp = (const float *)smem_raw;
        for (int s = 0; s < N.n_steps; ++s) {
            const KwsResStepF32 &k = N.st[s];
            const KwsResGeom &g = k.g;
            float *dbase;
            if (g.d_base >= 0) {
                float *img = wbase + g.d_base;
                for (int i = lane * 16; i < g.d_bytes; i += 64 * 16) *(float4 *)((unsigned char *)img + i) = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                WAVE_SYNC();
                dbase = img + g.d_off;
            } else dbase = handoff + (size_t)(ci - ci0) * N.out_n;
            const int dpitch = g.d_pitch;
            const int out_c = g.out_c, n_items = g.pool_h * g.pool_w * out_c;
            if (g.kind == KWS_RES_CONV) {
                const float *wb = k.w;                                // HBM, unless staged
                if (k.w_lds) { wb = bp; bp += (out_c * g.kh * g.krow + 3) & ~3; }
                const float *bias = bp;
                bp += (out_c + 3) & ~3;
                const float *cur = wbase + g.a_base + g.a_off;
                const int krow = g.krow, xstep = g.sw * g.in_c, ystep = g.sh * g.a_pitch;
                for (int item = lane; item < n_items; item += 64) {
                    const int pos = item / out_c, oc = item - pos * out_c;
                    const int py = pos / g.pool_w, px = pos - py * g.pool_w;
                    const int cy0 = py * g.psh - g.ppt, cx0 = px * g.psw - g.ppl;
                    const int wy0 = max(0, -cy0), wy1 = min(g.ph, g.out_h - cy0), wx0 = max(0, -cx0), wx1 = min(g.pw, g.out_w - cx0);
                    const float *wrow = wb + oc * g.kh * krow;
                    const float bv = bias[oc];
                    float mx = -FLT_MAX, v = 0.0f;
                    for (int wy = wy0; wy < wy1; ++wy)
                        for (int wx = wx0; wx < wx1; ++wx) {
                            const float *xr = cur + (cy0 + wy) * ystep + (cx0 + wx) * xstep;
                            const float *wr = wrow;
                            float total = 0.0f;
                            for (int fy = 0; fy < g.kh; ++fy) {
                                for (int j = 0; j < krow; ++j) {
                                    const float prod = xr[j] * wr[j];
                                    total += prod;
                                }
                                xr += g.a_pitch;
                                wr += krow;
                            }
                            v = nnres_clamp(total + bv, k.act_min, k.act_max);
                            mx = mx < v ? v : mx;                               // std::max(mx, v)
                        }
                    dbase[py * dpitch + px * out_c + oc] = g.has_pool ? nnres_clamp(mx, k.pool_min, k.pool_max) : v;
                }
            } else if (g.kind == KWS_RES_DW) {
                const float *wb = k.w;                                // HBM, unless staged
                if (k.w_lds) { wb = bp; bp += (out_c * g.kh * g.krow + 3) & ~3; }
                const float *bias = bp;
                bp += (out_c + 3) & ~3;
                const float *cur = wbase + g.a_base + g.a_off;
                const int in_c = g.in_c, xstep = g.sw * in_c, ystep = g.sh * g.a_pitch, wrow = g.kw * out_c;
                for (int item = lane; item < n_items; item += 64) {
                    const int pos = item / out_c, oc = item - pos * out_c;
                    const int py = pos / g.pool_w, px = pos - py * g.pool_w;
                    const int cy0 = py * g.psh - g.ppt, cx0 = px * g.psw - g.ppl;
                    const int wy0 = max(0, -cy0), wy1 = min(g.ph, g.out_h - cy0), wx0 = max(0, -cx0), wx1 = min(g.pw, g.out_w - cx0);
                    const int ic = g.dm == 1 ? oc : oc / g.dm;
                    const float bv = bias[oc];
                    float mx = -FLT_MAX, v = 0.0f;
                    for (int wy = wy0; wy < wy1; ++wy)
                        for (int wx = wx0; wx < wx1; ++wx) {
                            const float *xr = cur + (cy0 + wy) * ystep + (cx0 + wx) * xstep + ic;
                            const float *wr = wb + oc;
                            float total = 0.0f;
                            for (int fy = 0; fy < g.kh; ++fy) {
                                for (int fx = 0; fx < g.kw; ++fx) {
                                    const float prod = xr[fx * in_c] * wr[fx * out_c];
                                    total += prod;
                                }
                                xr += g.a_pitch;
                                wr += wrow;
                            }
                            v = nnres_clamp(total + bv, k.act_min, k.act_max);
                            mx = mx < v ? v : mx;                               // std::max(mx, v)
                        }
                    dbase[py * dpitch + px * out_c + oc] = g.has_pool ? nnres_clamp(mx, k.pool_min, k.pool_max) : v;
                }
            } else {
                const float *pa = wbase + g.a_base + g.a_off, *pb = wbase + g.b_base + g.b_off;
                for (int item = lane; item < n_items; item += 64) {
                    const int pos = item / out_c, oc = item - pos * out_c;
                    const int py = pos / g.pool_w, px = pos - py * g.pool_w;
                    const int cy0 = py * g.psh - g.ppt, cx0 = px * g.psw - g.ppl;
                    const int wy0 = max(0, -cy0), wy1 = min(g.ph, g.out_h - cy0), wx0 = max(0, -cx0), wx1 = min(g.pw, g.out_w - cx0);
                    float mx = -FLT_MAX, v = 0.0f;
                    for (int wy = wy0; wy < wy1; ++wy)
                        for (int wx = wx0; wx < wx1; ++wx) {
                            const int y = cy0 + wy, e = (cx0 + wx) * out_c + oc;
                            v = nnres_clamp(pa[y * g.a_pitch + e] + pb[y * g.b_pitch + e], k.act_min, k.act_max);       // reference/add.h
                            mx = mx < v ? v : mx;
                        }
                    dbase[py * dpitch + px * out_c + oc] = g.has_pool ? nnres_clamp(mx, k.pool_min, k.pool_max) : v;
                }
            }
            WAVE_SYNC();
        }
    }
}

int kws_launch_nnres_f32_trunk(const KwsResPlanF32 &N, const float *features, int n_clips, float *handoff, int ci0, int ci1, const int *sel, int n_cu,
                               hipStream_t stream)
{
    const int nw = kws_nnres_f32_waves(N), n = ci1 - ci0;
    if (nw == 0) return (int)hipErrorInvalidValue;           // (kws_create refuses such a graph)
    if (n <= 0) return 0;
    const size_t smem = kws_nnres_f32_smem_bytes(N, nw);
    if (smem > 64 * 1024) {                    // opt in to more than the default 64 KB of dynamic LDS
        hipError_t e = hipFuncSetAttribute((const void *)kws_nnres_f32_trunk_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
        if (e != hipSuccess) return (int)e;
    }
    int grid = (n + nw - 1) / nw;
    if (grid > n_cu) grid = n_cu;              // one persistent workgroup per CU
    hipLaunchKernelGGL(kws_nnres_f32_trunk_kernel, dim3(grid), dim3(KWS_WAVE * nw), smem, stream, N, features, n_clips, handoff, ci0, ci1, sel);
    return (int)hipGetLastError();
}
