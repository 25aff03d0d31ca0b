// kws_nn2d_f32.hip -- kws_nn2d_f32_trunk_kernel: the CONV_2D [+ MAX_POOL_2D] blocks of a float32 2-D graph, in front of
// kws_dense_f32_kernel.  Replays reference/conv.h:28-99 and reference/pooling.h:189-237 in the reference's own order.
//
// The execution model of kws_nn2d_trunk_kernel (kws_nn2d_int8.hip): one wave per clip, persistent workgroups, the filters ([out_c][kh][kw * in_c], the
// tensor's own order) and biases of every block once per workgroup in LDS, two ping-pong images per wave, a lane per pooled output (py, px, oc).
// Every output is ONE chain -- total += input * filter over fy, then fx, then ic, product and sum rounded separately (the build has -ffp-contract=off and
// kws_device.h switches contraction off), then + bias, then the clamp -- and in an NHWC image the fx, ic steps of one fy are consecutive floats of one image
// row, in the chain's order.  Padding is +0.0f: the reference skips an out-of-image tap, the kernel adds 0 * w = +-0 to a chain that started at +0 and can
// therefore never hold -0, which changes nothing for a FINITE w (the plan refuses a non-finite weight).  Inputs may be anything: an in-image
// inf or NaN meets the same weights in the same order as in the reference.
// MAX_POOL_2D is std::max over the window's in-image values in the reference's order (filter_y, then filter_x; max = max < v ? v : max, so a NaN never
// wins and of two zeros the first stays), from numeric_limits::lowest(), then the pool's own clamp: the lane computes its window's convolutions in that
// order, each finished (bias, clamp) before it is compared.
#include <algorithm>

#include "kws_device.h"
#include "kws_nn2d.h"

__device__ __forceinline__ float nn2d_clamp(float x, float lo, float hi)   // ActivationFunctionWithMinMax: std::min(std::max(x, lo), hi)
{
    const float a = x < lo ? lo : x;
    return hi < a ? hi : a;
}

__global__ __launch_bounds__(KWS_WAVE * KWS_NN2D_WAVES_MAX) void kws_nn2d_f32_trunk_kernel(KwsNn2dPlanF32 N, const float *__restrict__ features, int n_clips,
                                                                                          float *__restrict__ handoff, int ci0, int ci1,
                                                                                          const int *__restrict__ sel)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), n_waves = blockDim.x >> 6;

    // ---- shared: filters and biases of every block, in block order ------------------------------------------------
    float *sp = (float *)smem_raw;
    int img_b[2] = { 0, 0 };                           // bytes; block b reads image b & 1
    for (int b = 0; b < N.n_blocks; ++b) {
        const KwsConv2dBlockF32 &k = N.blk[b];
        const int nw = k.g.out_c * k.g.kh * k.g.krow;
        for (int i = threadIdx.x; i < nw; i += blockDim.x) sp[i] = k.w[i];
        sp += (nw + 3) & ~3;
        for (int i = threadIdx.x; i < k.g.out_c; i += blockDim.x) sp[i] = k.bias[i];
        sp += (k.g.out_c + 3) & ~3;
        img_b[b & 1] = max(img_b[b & 1], kws_nn2d_img_bytes(k.g, 4));
    }
    float *const imgA = (float *)((unsigned char *)sp + (size_t)wave * (img_b[0] + img_b[1]));
    float *const imgB = (float *)((unsigned char *)imgA + img_b[0]);
    __syncthreads();

    const int n_sel = min(sel_count(sel, n_clips), ci1);
    for (int ci = ci0 + blockIdx.x * n_waves + wave; ci < n_sel; ci += gridDim.x * n_waves) {
        const int clip = sel_clip(sel, ci);
        // ---- stage the feature matrix [in_h][in_w][in_c] behind its zero padding -------------------------------------
        {
            const KwsConv2dGeom &g = N.blk[0].g;
            for (int i = lane * 16; i < kws_nn2d_img_bytes(g, 4); i += 64 * 16) *(float4 *)((unsigned char *)imgA + i) = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            WAVE_SYNC();
            const float *src = features + (size_t)clip * N.n_features;
            const int row = g.in_w * g.in_c;
            for (int i = lane; i < g.in_h * row; i += 64) {
                const int y = i / row, x = i - y * row;
                imgA[(y + g.pad_t) * g.img_pitch + g.pad_l * g.in_c + x] = src[i];
            }
            WAVE_SYNC();
        }
        float *cur = imgA, *nxt = imgB;
        const float *bp = (const float *)smem_raw;
        for (int b = 0; b < N.n_blocks; ++b) {
            const KwsConv2dBlockF32 &k = N.blk[b];
            const KwsConv2dGeom &g = k.g;
            const float *wb = bp;
            bp += (g.out_c * g.kh * g.krow + 3) & ~3;
            const float *bias = bp;
            bp += (g.out_c + 3) & ~3;
            const bool last = (b + 1 == N.n_blocks);
            float *dbase;
            int dpitch;
            if (!last) {
                const KwsConv2dGeom &ng = N.blk[b + 1].g;
                for (int i = lane * 16; i < kws_nn2d_img_bytes(ng, 4); i += 64 * 16) *(float4 *)((unsigned char *)nxt + i) = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                WAVE_SYNC();
                dbase = nxt + ng.pad_t * ng.img_pitch + ng.pad_l * g.out_c;
                dpitch = ng.img_pitch;
            } else {
                dbase = handoff + (size_t)(ci - ci0) * N.out_n;
                dpitch = g.pool_w * g.out_c;
            }
            const int out_c = g.out_c, n_items = g.pool_h * g.pool_w * out_c;
            const int krow = g.krow, xstep = g.sw * g.in_c, ystep = g.sh * g.img_pitch;
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
                            xr += g.img_pitch;
                            wr += krow;
                        }
                        v = nn2d_clamp(total + bv, k.conv_min, k.conv_max);
                        mx = mx < v ? v : mx;                               // std::max(mx, v)
                    }
                dbase[py * dpitch + px * out_c + oc] = g.has_pool ? nn2d_clamp(mx, k.pool_min, k.pool_max) : v;
            }
            WAVE_SYNC();
            float *tmp = cur; cur = nxt; nxt = tmp;
        }
    }
}

int kws_launch_nn2d_f32_trunk(const KwsNn2dPlanF32 &N, const float *features, int n_clips, float *handoff, int ci0, int ci1, const int *sel, int n_cu,
                              hipStream_t stream)
{
    const int nw = kws_nn2d_f32_waves(N), n = ci1 - ci0;
    if (nw == 0) return (int)hipErrorInvalidValue;           // (kws_create refuses such a graph)
    if (n <= 0) return 0;
    const size_t smem = kws_nn2d_f32_smem_bytes(N, nw);
    if (smem > 64 * 1024) {                    // opt in to more than the default 64 KB of dynamic LDS
        hipError_t e = hipFuncSetAttribute((const void *)kws_nn2d_f32_trunk_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
        if (e != hipSuccess) return (int)e;
    }
    int grid = (n + nw - 1) / nw;
    if (grid > n_cu) grid = n_cu;              // one persistent workgroup per CU
    hipLaunchKernelGGL(kws_nn2d_f32_trunk_kernel, dim3(grid), dim3(KWS_WAVE * nw), smem, stream, N, features, n_clips, handoff, ci0, ci1, sel);
    return (int)hipGetLastError();
}
