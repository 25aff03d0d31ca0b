// kws_nn_int8.hip -- the int8 network: kws_nn_kernel<MAXW, TRUNK, SD> (generic, kws_nn_int8_generic.h: any chain of conv blocks, with its head or as the
// trunk of a dense stack, stride 1 or strided / dilated; un-pooled CONV_2D on the matrix cores, depthwise in registers, the rest on v_dot4),
// kws_nn_mfma_kernel (the two-block shape entirely on the matrix cores) and kws_cmvn_nn_kernel (cmvnw + quantise [+ network] for the stage API /
// continuous mode).  Replaces the EON-compiled TFLite-Micro graph (MODEL/tflite-model/trained_model_compiled.cpp:312-328).
#include "kws_device.h"
#include <cstdio>
#include <cstdlib>

#include "kws_nn_int8_dev.h"
#include "kws_nn_int8_generic.h"

#include "kws_dense_i8.h"
#include "kws_nn2d.h"
#include "kws_nnres.h"

template <int CP>
__global__ __launch_bounds__(KWS_WAVE * KWS_NN_WAVES) void kws_nn_mfma_kernel(KwsNnPlan N, const int8_t *__restrict__ q_in, int n_clips,
                                                                              float *__restrict__ scores, NnTaps taps)
{
    __shared__ __attribute__((aligned(16))) int8_t s_lut1[32 * 256];
    __shared__ __attribute__((aligned(16))) int8_t s_lut2[16 * 256];
    __shared__ __attribute__((aligned(16))) int8_t s_act1[KWS_NN_WAVES][KWS_A1_ROWS * CP];
    __shared__ __attribute__((aligned(16))) int8_t s_act2[KWS_NN_WAVES][KWS_A2_ROWS * 32];
    __shared__ int s_vec[KWS_NN_WAVES][64];
    __shared__ __attribute__((aligned(16))) unsigned char s_head[KWS_HEAD_BYTES];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));    // uniform: per-wave addresses stay in scalar registers
    const KwsConvBlock &k1 = N.blk[0], &k2 = N.blk[1];
    const NnHeadTab head = nn_head_stage(N, s_head);
    for (int i = threadIdx.x * 4; i < k1.out_c * 256; i += blockDim.x * 4) *(int *)(s_lut1 + i) = *(const int *)(k1.add_lut + i);
    for (int i = threadIdx.x * 4; i < k2.out_c * 256; i += blockDim.x * 4) *(int *)(s_lut2 + i) = *(const int *)(k2.add_lut + i);
    int8_t *act1 = s_act1[wave], *act2 = s_act2[wave];
    nn_mfma_fill_padding<CP>(N, act1, act2, lane);
    NnMfmaCtx<CP> ctx;
    nn_mfma_init<CP>(ctx, N, lane);
    __syncthreads();
    const int F = N.n_features;
    const unsigned inv_c = (1u << 20) / (unsigned)k1.in_c + 1u;          // i / in_c == (i * inv_c) >> 20 for i < n_features <= 4096
    const int n_sel = sel_count(taps.sel, n_clips);
    for (int ci = blockIdx.x * KWS_NN_WAVES + wave; ci < n_sel; ci += gridDim.x * KWS_NN_WAVES) {
        const int clip = sel_clip(taps.sel, ci);
        // ---- int8 input tensor [time][in_c] -> LDS rows of CP bytes at row (time + pad_left) --------------------
        const int8_t *src = q_in + (size_t)clip * F;
        if ((k1.in_c & 3) == 0) {                          // four channels per copy (feature vector and rows 4-byte aligned)
            for (int i = lane * 4; i < F; i += 64 * 4) {
                const int tt = (int)(((unsigned)i * inv_c) >> 20), c = i - tt * k1.in_c;
                *(int *)(act1 + (tt + k1.pad_left) * CP + c) = *(const int *)(src + i);
            }
        } else {
            for (int i = lane; i < F; i += 64) {
                const int tt = (int)(((unsigned)i * inv_c) >> 20), c = i - tt * k1.in_c;       // i / in_c
                act1[(tt + k1.pad_left) * CP + c] = src[i];
            }
        }
        WAVE_SYNC();
        nn_mfma_clip<CP>(ctx, N, head, act1, act2, s_vec[wave], s_lut1, s_lut2, lane, clip, scores, taps);
    }
}

// ---------------------------------------------------------------------------------------------------------
//  Kernel 2': cmvnw (processing.hpp:326-389) + input quantisation (ei_run_classifier.h:436-444) [+ the network when
//  FUSE and the graph fits the matrix-core path].  One wave per window, 4 waves per workgroup.
//  CMVN: cmvn_columns<13, 16> (shared with kws_mfcc_kernel).
// ---------------------------------------------------------------------------------------------------------
template <bool FUSE>
__global__ __launch_bounds__(KWS_WAVE * KWS_NN_WAVES, 2) void kws_cmvn_nn_kernel(KwsDspPlan P, KwsNnPlan N, const float *__restrict__ mfcc,
                                                                              int n_clips, float *__restrict__ features,
                                                                              int8_t *__restrict__ q_out, float *__restrict__ scores,
                                                                              NnTaps taps)
{
    __shared__ int s_map[KWS_MAXPROW];                                    // numpy::pad_1d_symmetric row map (numpy.hpp:479-541)
    __shared__ float s_mfcc[KWS_NN_WAVES][KWS_MAXF * KWS_NF_MAX];       // cepstra before CMVN, [frame][coef] (coef <= filters)
    __shared__ __attribute__((aligned(16))) int s_off[KWS_NN_WAVES][2 * KWS_ZF];   // cmvn_columns' row-offset table (same bound as in kws_mfcc_kernel)
    __shared__ __attribute__((aligned(16))) int8_t s_lut1[FUSE ? 32 * 256 : 16];
    __shared__ __attribute__((aligned(16))) int8_t s_lut2[FUSE ? 16 * 256 : 16];
    __shared__ __attribute__((aligned(16))) int8_t s_act1[KWS_NN_WAVES][FUSE ? KWS_A1_ROWS * 16 : 16];
    __shared__ __attribute__((aligned(16))) int8_t s_act2[KWS_NN_WAVES][FUSE ? KWS_A2_ROWS * 32 : 16];
    __shared__ int s_vec[KWS_NN_WAVES][FUSE ? 64 : 1];
    __shared__ __attribute__((aligned(16))) unsigned char s_head[FUSE ? KWS_HEAD_BYTES : 16];
    NnHeadTab head = { nullptr, nullptr, nullptr, nullptr };
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));    // uniform: per-wave addresses stay in scalar registers
    const int nfr = P.n_frames, ncep = P.n_cepstral, nfeat = nfr * ncep;
    const int prow = nfr + 2 * P.pad;
    for (int i = threadIdx.x; i < prow; i += blockDim.x) s_map[i] = P.pad_map[i];
    NnMfmaCtx<16> ctx;
    int8_t *act1 = s_act1[wave], *act2 = s_act2[wave];
    if constexpr (FUSE) {
        head = nn_head_stage(N, s_head);
        const KwsConvBlock &k1 = N.blk[0], &k2 = N.blk[1];
        for (int i = threadIdx.x * 4; i < k1.out_c * 256; i += blockDim.x * 4) *(int *)(s_lut1 + i) = *(const int *)(k1.add_lut + i);
        for (int i = threadIdx.x * 4; i < k2.out_c * 256; i += blockDim.x * 4) *(int *)(s_lut2 + i) = *(const int *)(k2.add_lut + i);
        nn_mfma_fill_padding<16>(N, act1, act2, lane);
        nn_mfma_init<16>(ctx, N, lane);
    }
    __syncthreads();
    float *mf = s_mfcc[wave];
    const int win = P.win_size;
    const float in_scale = N.in_scale;
    const int in_zp = N.in_zp;

    const int n_sel = sel_count(taps.sel, n_clips);
    for (int ci = blockIdx.x * KWS_NN_WAVES + wave; ci < n_sel; ci += gridDim.x * KWS_NN_WAVES) {
        const int clip = sel_clip(taps.sel, ci);
        const float *src = mfcc + (size_t)clip * nfeat;
        if (P.ring_rows) {
            const unsigned inv = (1u << 20) / (unsigned)ncep + 1u;          // i / ncep for i < 4096, ncep <= 64
            for (int i = lane; i < nfeat; i += 64) {
                const int r = (int)(((unsigned)i * inv) >> 20);
                mf[i] = src[ring_in_row(P, r) * ncep + (i - r * ncep)];
            }
        } else {
            for (int i = lane; i < nfeat; i += 64) mf[i] = src[i];
        }
        WAVE_SYNC();
        cmvn_columns<13, 16>(mf, ncep, s_map, s_off[wave], lane, nfr, ncep, prow, win, [&](int row, int c, float o) {
            const int idx = row * ncep + c;
            if (features) features[(size_t)clip * nfeat + idx] = o;
            const int8_t qb = quantize_feature(o, in_scale, in_zp);
            if (q_out) q_out[(size_t)clip * nfeat + idx] = qb;
            if constexpr (FUSE) act1[(row + N.blk[0].pad_left) * 16 + c] = qb;
        });
        WAVE_SYNC();
        if constexpr (FUSE) nn_mfma_clip<16>(ctx, N, head, act1, act2, s_vec[wave], s_lut1, s_lut2, lane, clip, scores, taps);
    }
}

// ---------------------------------------------------------------------------------------------------------
//  launchers (called from kws_api.cpp)
// ---------------------------------------------------------------------------------------------------------

long long *kws_dev_nn_prof = nullptr;   // development aid (tools/gpu_nn_phase_profile.py)
int kws_force_scalar_nn = 0;   // tests: run the generic (dot4) kernel even when the matrix-core kernel applies
int kws_nn_uses_mfma(const KwsNnPlan &N) { return nn_fits_mfma(N) && !kws_force_scalar_nn; }

// cmvnw + quantise (+ the network when it fits the matrix-core path and scores != NULL).  Returns 1 in *ran_nn if the
// network ran inside this launch.
int kws_launch_cmvn_nn(const KwsDspPlan &P, const KwsNnPlan &N, const float *mfcc, int n_clips, float *features, int8_t *q_out,
                       float *scores, int8_t *tap_pooled, int pooled_stride, int8_t *tap_fc, int8_t *tap_out_q, int grid_cap,
                       int *ran_nn, hipStream_t stream, const int *sel)
{
    (void)hipGetLastError();      // the status returned below is this launch's, not a stale error of an earlier call
    *ran_nn = 0;
    if (n_clips <= 0) return 0;
    int grid = (n_clips + KWS_NN_WAVES - 1) / KWS_NN_WAVES;
    if (grid > grid_cap) grid = grid_cap;
    NnTaps taps = { tap_pooled, pooled_stride, tap_fc, tap_out_q, kws_dev_nn_prof, sel };
    if (scores && nn_fits_mfma(N) && N.blk[0].in_cpad == 16 && !kws_force_scalar_nn) {      // (64-byte rows: separate network launch)
        hipLaunchKernelGGL((kws_cmvn_nn_kernel<true>), dim3(grid), dim3(KWS_WAVE * KWS_NN_WAVES), 0, stream, P, N, mfcc, n_clips,
                           features, q_out, scores, taps);
        *ran_nn = 1;
    } else {
        hipLaunchKernelGGL((kws_cmvn_nn_kernel<false>), dim3(grid), dim3(KWS_WAVE * KWS_NN_WAVES), 0, stream, P, N, mfcc, n_clips,
                           features, q_out, scores, taps);
    }
    return (int)hipGetLastError();
}
size_t kws_nn_smem_bytes(const KwsNnPlan &N, int n_waves)
{
    size_t s = (size_t)nn_head_fcw_bytes(N) + ((KWS_HEAD_REST + 15) & ~15);
    int act[2] = { 0, 0 };
    for (int b = 0; b < N.n_blocks; ++b) {
        const KwsConvBlock &k = N.blk[b];
        s += ((size_t)k.w_bytes + 15) & ~(size_t)15;
        s += k.has_lut ? (size_t)k.out_c * 256 : 0;
        s += (size_t)k.out_c * 16;                      // requantisation constants
        const int ab = nn_rows_sd(k) * k.in_cpad;             // (= nn_rows(k) for a stride-1, dilation-1 block)
        act[b & 1] = ab > act[b & 1] ? ab : act[b & 1];
    }
    return s + (size_t)n_waves * (((act[0] + 15) & ~15) + ((act[1] + 15) & ~15) + nn_fcx_bytes(N) + 64 * 4);
}

// The form of kws_nn_kernel that serves a graph, chosen ONCE per call: the pointer this returns is the one hipFuncSetAttribute opts in to large LDS and
// the one nn_launch launches.  trunk: the graph has a dense stack behind its conv blocks; sd: some block is strided or dilated; at most
// twelve waves per workgroup take the 168-register build.
static const void *nn_kernel_for(bool trunk, bool sd, int nw)
{
    static const void *const tab[2][2][2] = {
        { { (const void *)kws_nn_kernel<16, false, false>, (const void *)kws_nn_kernel<12, false, false> },
          { (const void *)kws_nn_kernel<16, false, true>, (const void *)kws_nn_kernel<12, false, true> } },
        { { (const void *)kws_nn_kernel<16, true, false>, (const void *)kws_nn_kernel<12, true, false> },
          { (const void *)kws_nn_kernel<16, true, true>, (const void *)kws_nn_kernel<12, true, true> } } };
    return tab[trunk][sd][nw <= 12];
}
// (every form has the one argument list; a form ignores the arguments that are not its own)
static void nn_launch(const void *fn, int grid, int nw, size_t smem, hipStream_t stream, const KwsNnPlan &N, const int8_t *q_in, int n_clips,
                      float *scores, int8_t *handoff, int ci0, int ci1, NnTaps taps)
{
    void *args[] = { const_cast<KwsNnPlan *>(&N), &q_in, &n_clips, &scores, &handoff, &ci0, &ci1, &taps };
    (void)hipLaunchKernel(fn, dim3(grid), dim3(KWS_WAVE * nw), args, smem, stream);
}

// A graph with a dense stack: the conv blocks (if any) in the trunk form of the generic kernel, chunk by chunk of the hand-off buffer, each chunk followed
// by kws_dense_i8_kernel over the same list entries.
static int launch_dense_i8(const KwsNnPlan &N, const int8_t *q_in, int n_clips, float *scores, const NnTaps &taps, int grid_cap, hipStream_t stream)
{
    const KwsDensePlan &D = *N.dense;
    const size_t smem = kws_dense_i8_smem_bytes(D);
    if (smem > 64 * 1024) {
        hipError_t e = hipFuncSetAttribute((const void *)kws_dense_i8_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
        if (e != hipSuccess) return (int)e;
    }
    auto dense_grid = [&](int n) { const int g = (n + 16 * KWS_DENSE_WAVES - 1) / (16 * KWS_DENSE_WAVES); return g > grid_cap ? grid_cap : g; };
    const KwsNn2dPlan *const trunk2d = N.handoff->trunk2d;     // a 2-D graph: kws_nn2d_trunk_kernel fills the hand-off
    const KwsResPlan *const trunkres = N.handoff->trunkres;     // a residual graph: kws_nnres_trunk_kernel fills the hand-off
    if (N.n_blocks == 0 && !trunk2d && !trunkres) {
        hipLaunchKernelGGL(kws_dense_i8_kernel, dim3(dense_grid(n_clips)), dim3(KWS_WAVE * KWS_DENSE_WAVES), smem, stream, D, q_in, 1, 0, n_clips, n_clips, scores, taps);
        return (int)hipGetLastError();
    }
    int8_t *ho = (int8_t *)kws_handoff_for(N.handoff, (void *)stream);
    if (!ho) return (int)hipErrorOutOfMemory;
    int nw = KWS_NN_WAVES_MAX;
    while (nw > KWS_NN_WAVES && kws_nn_smem_bytes(N, nw) > 158 * 1024) --nw;
    const size_t tsmem = kws_nn_smem_bytes(N, nw);
    const void *fn = nn_kernel_for(true, kws_nn_strided(N) != 0, nw);
    if (!trunk2d && !trunkres && tsmem > 64 * 1024) {
        hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)tsmem);
        if (e != hipSuccess) return (int)e;
    }
    const int chunk = (int)(N.handoff->bytes / (size_t)N.fc_in);            // >= 4096 clips at KWS_HANDOFF_BYTES
    for (int c0 = 0; c0 < n_clips; c0 += chunk) {
        const int c1 = n_clips - c0 > chunk ? c0 + chunk : n_clips, n = c1 - c0;
        int grid = (n + nw - 1) / nw;
        if (grid > grid_cap / 4) grid = grid_cap / 4;                         // grid_cap = 4 workgroups per CU; one persistent workgroup per CU
        if (trunk2d) {
            if (!kws_launch_nn2d_trunk) return (int)hipErrorInvalidDeviceFunction;      // (linked without kws_nn2d_int8.hip: kws_nn2d.h)
            const int rc = kws_launch_nn2d_trunk(*trunk2d, q_in, n_clips, ho, c0, c1, taps.pooled, taps.pooled_stride, taps.sel, grid_cap / 4, stream);
            if (rc) return rc;
        } else if (trunkres) {
            if (!kws_launch_nnres_trunk) return (int)hipErrorInvalidDeviceFunction;     // (linked without kws_nnres_int8.hip: kws_nnres.h)
            const int rc = kws_launch_nnres_trunk(*trunkres, q_in, n_clips, ho, c0, c1, taps.pooled, taps.pooled_stride, taps.sel, grid_cap / 4, stream);
            if (rc) return rc;
        } else nn_launch(fn, grid, nw, tsmem, stream, N, q_in, n_clips, nullptr, ho, c0, c1, taps);
        hipLaunchKernelGGL(kws_dense_i8_kernel, dim3(dense_grid(n)), dim3(KWS_WAVE * KWS_DENSE_WAVES), smem, stream, D, (const int8_t *)ho, 0, c0, c1, n_clips, scores, taps);
        const int rc = (int)hipGetLastError();
        if (rc) return rc;
    }
    return 0;
}

int kws_launch_nn(const KwsNnPlan &N, const int8_t *q_in, int n_clips, float *scores, int8_t *tap_pooled,
                  int pooled_stride, int8_t *tap_fc, int8_t *tap_out_q, int grid_cap, hipStream_t stream, const int *sel)
{
    (void)hipGetLastError();      // the status returned below is this launch's, not a stale error of an earlier call
    if (n_clips <= 0) return 0;
    int grid = (n_clips + KWS_NN_WAVES - 1) / KWS_NN_WAVES;
    if (grid > grid_cap) grid = grid_cap;
    NnTaps taps = { tap_pooled, pooled_stride, tap_fc, tap_out_q, kws_dev_nn_prof, sel };
    if (kws_nn_dense(N)) return launch_dense_i8(N, q_in, n_clips, scores, taps, grid_cap, stream);
    if (nn_fits_mfma(N) && !kws_force_scalar_nn) {
        if (N.blk[0].in_cpad == 16)
            hipLaunchKernelGGL(kws_nn_mfma_kernel<16>, dim3(grid), dim3(KWS_WAVE * KWS_NN_WAVES), 0, stream, N, q_in, n_clips, scores, taps);
        else
            hipLaunchKernelGGL(kws_nn_mfma_kernel<64>, dim3(grid), dim3(KWS_WAVE * KWS_NN_WAVES), 0, stream, N, q_in, n_clips, scores, taps);
        return (int)hipGetLastError();
    }
    // generic kernel (168 VGPRs: three waves per SIMD): one persistent workgroup per CU with as many waves as the LDS holds (they
    // share the weights and tables), up to twelve
    int nw = KWS_NN_WAVES_MAX, per_cu = 1;
    while (nw > KWS_NN_WAVES && kws_nn_smem_bytes(N, nw) > 158 * 1024) --nw;
    if (const char *ev = KWS_DEV_ENV("KWS_DEV_NN_WAVES")) { int a = 0, b2 = 0; if (sscanf(ev, "%d,%d", &a, &b2) == 2 && a >= 1 && a <= KWS_NN_WAVES_MAX && b2 >= 1) { nw = a; per_cu = b2; } }   // development aid (occupancy experiments)
    const size_t smem = kws_nn_smem_bytes(N, nw);
    grid = (n_clips + nw - 1) / nw;
    if (grid > (grid_cap / 4) * per_cu) grid = (grid_cap / 4) * per_cu;          // grid_cap = 4 workgroups per CU
    const void *fn = nn_kernel_for(false, kws_nn_strided(N) != 0, nw);
    if (smem > 64 * 1024) {                    // wide models: opt in to more than the default 64 KB of dynamic LDS
        hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
        if (e != hipSuccess) return (int)e;
    }
    nn_launch(fn, grid, nw, smem, stream, N, q_in, n_clips, scores, nullptr, 0, 0, taps);
    return (int)hipGetLastError();
}

