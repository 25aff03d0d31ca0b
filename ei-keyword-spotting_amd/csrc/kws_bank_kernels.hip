// kws_bank_kernels.hip -- the networks of a bank (kws_bank.cpp; contract in include/kws/kws.h) behind ONE float feature matrix:
// kws_bank_nn_mfma_kernel (every int8 member of the two-block matrix-core shape in one launch per activation-row width, quantising the
// features on load) and kws_bank_quantize_kernel (the int8 input tensors of the other int8 members in one pass over the matrix); and the
// routed forms of both (kws_bank_nn_mfma_routed_kernel, kws_bank_quantize_routed_kernel), which serve each member its own list of rows.
// The network itself is kws_nn_int8_dev.h's, unchanged: a member's scores are those of its own kws_nn_mfma_kernel launch bit for bit.
#include "kws_device.h"

#include "kws_nn_int8_dev.h"
#include "kws_bank.h"

// ---------------------------------------------------------------------------------------------------------
//  Grid (clip tiles, member): blockIdx.y picks the member's record in HBM (its plan and input quantisation; uniform over the
//  workgroup, so the plan is read through the scalar cache as kws_nn_mfma_kernel reads its by-value copy) and its score buffer in
//  the launch arguments.  The workgroup stages that member's head and ADD tables once; each wave then takes clips: the clip's float
//  feature row is read once and quantised (quantize_feature, the expression of every other path) straight into the act1 rows -- no
//  int8 tensor goes through HBM -- and nn_mfma_clip does the rest.  LDS and registers: those of kws_nn_mfma_kernel<CP>.
// ---------------------------------------------------------------------------------------------------------
template <int CP>
__global__ __launch_bounds__(KWS_WAVE * KWS_NN_WAVES) void kws_bank_nn_mfma_kernel(const KwsBankRec *__restrict__ recs, KwsBankOut out,
                                                                                   const float *__restrict__ features, int n_clips)
{
    __shared__ __attribute__((aligned(16))) int8_t s_lut1[32 * 256];
    __shared__ __attribute__((aligned(16))) int8_t s_lut2[16 * 256];
    __shared__ __attribute__((aligned(16))) int8_t s_act1[KWS_NN_WAVES][KWS_A1_ROWS * CP];
    __shared__ __attribute__((aligned(16))) int8_t s_act2[KWS_NN_WAVES][KWS_A2_ROWS * 32];
    __shared__ int s_vec[KWS_NN_WAVES][64];
    __shared__ __attribute__((aligned(16))) unsigned char s_head[KWS_HEAD_BYTES];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));    // uniform: per-wave addresses stay in scalar registers
    const int slot = (int)blockIdx.y;
    const KwsBankRec &R = recs[out.rec[slot]];
    const KwsNnPlan &N = R.N;
    float *__restrict__ scores = out.scores[slot];
    const KwsConvBlock &k1 = N.blk[0], &k2 = N.blk[1];
    const NnHeadTab head = nn_head_stage(N, s_head);
    for (int i = threadIdx.x * 4; i < k1.out_c * 256; i += blockDim.x * 4) *(int *)(s_lut1 + i) = *(const int *)(k1.add_lut + i);
    for (int i = threadIdx.x * 4; i < k2.out_c * 256; i += blockDim.x * 4) *(int *)(s_lut2 + i) = *(const int *)(k2.add_lut + i);
    int8_t *act1 = s_act1[wave], *act2 = s_act2[wave];
    nn_mfma_fill_padding<CP>(N, act1, act2, lane);
    NnMfmaCtx<CP> ctx;
    nn_mfma_init<CP>(ctx, N, lane);
    __syncthreads();
    const int F = N.n_features, in_c = k1.in_c, pad_left = k1.pad_left;
    const float in_scale = R.in_scale;
    const int in_zp = R.in_zp;
    const unsigned inv_c = (1u << 20) / (unsigned)in_c + 1u;             // i / in_c == (i * inv_c) >> 20 for i < n_features <= 4096
    // four channels per load and store where the rows allow it (feature rows and activation rows 16- / 4-byte aligned)
    const bool quads = (in_c & 3) == 0 && ((uintptr_t)features & 15) == 0;
    const NnTaps taps = { nullptr, 0, nullptr, nullptr, nullptr, nullptr };
    for (int clip = blockIdx.x * KWS_NN_WAVES + wave; clip < n_clips; clip += gridDim.x * KWS_NN_WAVES) {
        // ---- float feature row [time][in_c] -> int8 LDS rows of CP bytes at row (time + pad_left) ------------------
        const float *src = features + (size_t)clip * F;
        if (quads) {
            for (int i = lane * 4; i < F; i += 64 * 4) {
                const float4 v = *(const float4 *)(src + i);
                const int tt = (int)(((unsigned)i * inv_c) >> 20), c = i - tt * in_c;
                const int w = (quantize_feature(v.x, in_scale, in_zp) & 0xff) | ((quantize_feature(v.y, in_scale, in_zp) & 0xff) << 8) |
                              ((quantize_feature(v.z, in_scale, in_zp) & 0xff) << 16) | (int)((unsigned)(quantize_feature(v.w, in_scale, in_zp) & 0xff) << 24);
                *(int *)(act1 + (tt + pad_left) * CP + c) = w;
            }
        } else {
            for (int i = lane; i < F; i += 64) {
                const int tt = (int)(((unsigned)i * inv_c) >> 20), c = i - tt * in_c;       // i / in_c
                act1[(tt + pad_left) * CP + c] = quantize_feature(src[i], in_scale, in_zp);
            }
        }
        WAVE_SYNC();
        nn_mfma_clip<CP>(ctx, N, head, act1, act2, s_vec[wave], s_lut1, s_lut2, lane, clip, scores, taps);
    }
}

// The routed form, a sibling: the same (tiles, member) grid, sized by the longest list of the launch.  Slot blockIdx.y walks
// lists.list[blockIdx.y] -- [0] = how many, then the clips, ascending -- instead of 0 .. n_clips - 1: a wave's position in the list is
// uniform, so the clip index is one scalar load, and everything behind it (LDS, staging, nn_mfma_clip) is the kernel above.
template <int CP>
__global__ __launch_bounds__(KWS_WAVE * KWS_NN_WAVES) void kws_bank_nn_mfma_routed_kernel(const KwsBankRec *__restrict__ recs, KwsBankOut out, KwsBankLists lists,
                                                                                          const float *__restrict__ features)
{
    __shared__ __attribute__((aligned(16))) int8_t s_lut1[32 * 256];
    __shared__ __attribute__((aligned(16))) int8_t s_lut2[16 * 256];
    __shared__ __attribute__((aligned(16))) int8_t s_act1[KWS_NN_WAVES][KWS_A1_ROWS * CP];
    __shared__ __attribute__((aligned(16))) int8_t s_act2[KWS_NN_WAVES][KWS_A2_ROWS * 32];
    __shared__ int s_vec[KWS_NN_WAVES][64];
    __shared__ __attribute__((aligned(16))) unsigned char s_head[KWS_HEAD_BYTES];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));    // uniform: per-wave addresses stay in scalar registers
    const int slot = (int)blockIdx.y;
    const KwsBankRec &R = recs[out.rec[slot]];
    const KwsNnPlan &N = R.N;
    float *__restrict__ scores = out.scores[slot];
    const KwsConvBlock &k1 = N.blk[0], &k2 = N.blk[1];
    const NnHeadTab head = nn_head_stage(N, s_head);
    for (int i = threadIdx.x * 4; i < k1.out_c * 256; i += blockDim.x * 4) *(int *)(s_lut1 + i) = *(const int *)(k1.add_lut + i);
    for (int i = threadIdx.x * 4; i < k2.out_c * 256; i += blockDim.x * 4) *(int *)(s_lut2 + i) = *(const int *)(k2.add_lut + i);
    int8_t *act1 = s_act1[wave], *act2 = s_act2[wave];
    nn_mfma_fill_padding<CP>(N, act1, act2, lane);
    NnMfmaCtx<CP> ctx;
    nn_mfma_init<CP>(ctx, N, lane);
    __syncthreads();
    const int F = N.n_features, in_c = k1.in_c, pad_left = k1.pad_left;
    const float in_scale = R.in_scale;
    const int in_zp = R.in_zp;
    const unsigned inv_c = (1u << 20) / (unsigned)in_c + 1u;             // i / in_c == (i * inv_c) >> 20 for i < n_features <= 4096
    // four channels per load and store where the rows allow it (feature rows and activation rows 16- / 4-byte aligned)
    const bool quads = (in_c & 3) == 0 && ((uintptr_t)features & 15) == 0;
    const NnTaps taps = { nullptr, 0, nullptr, nullptr, nullptr, nullptr };
    const int *__restrict__ list = lists.list[slot];
    const int n_list = list[0];
    for (int ci = blockIdx.x * KWS_NN_WAVES + wave; ci < n_list; ci += gridDim.x * KWS_NN_WAVES) {
        const int clip = __builtin_amdgcn_readfirstlane(list[1 + ci]);
        // ---- float feature row [time][in_c] -> int8 LDS rows of CP bytes at row (time + pad_left) ------------------
        const float *src = features + (size_t)clip * F;
        if (quads) {
            for (int i = lane * 4; i < F; i += 64 * 4) {
                const float4 v = *(const float4 *)(src + i);
                const int tt = (int)(((unsigned)i * inv_c) >> 20), c = i - tt * in_c;
                const int w = (quantize_feature(v.x, in_scale, in_zp) & 0xff) | ((quantize_feature(v.y, in_scale, in_zp) & 0xff) << 8) |
                              ((quantize_feature(v.z, in_scale, in_zp) & 0xff) << 16) | (int)((unsigned)(quantize_feature(v.w, in_scale, in_zp) & 0xff) << 24);
                *(int *)(act1 + (tt + pad_left) * CP + c) = w;
            }
        } else {
            for (int i = lane; i < F; i += 64) {
                const int tt = (int)(((unsigned)i * inv_c) >> 20), c = i - tt * in_c;       // i / in_c
                act1[(tt + pad_left) * CP + c] = quantize_feature(src[i], in_scale, in_zp);
            }
        }
        WAVE_SYNC();
        nn_mfma_clip<CP>(ctx, N, head, act1, act2, s_vec[wave], s_lut1, s_lut2, lane, clip, scores, taps);
    }
}

// the int8 input tensors of up to KWS_BANK_MAX members from one read of the feature matrix: q[j][i] = quantize_feature(f[i], scale j, zp j)
__global__ __launch_bounds__(256) void kws_bank_quantize_kernel(const float *__restrict__ f, size_t n, KwsBankQuant Q)
{
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const float v = f[i];
        for (int j = 0; j < Q.n; ++j) Q.q[j][i] = quantize_feature(v, Q.scale[j], Q.zp[j]);
    }
}

// The routed form: grid (blocks, member slot); slot j's tensor gets the rows its list names, row_len values each, and no other byte.
__global__ __launch_bounds__(256) void kws_bank_quantize_routed_kernel(const float *__restrict__ f, int row_len, KwsBankQuant Q, KwsBankLists lists)
{
    const int j = (int)blockIdx.y;
    const int *__restrict__ list = lists.list[j];
    const float scale = Q.scale[j];
    const int zp = Q.zp[j];
    int8_t *__restrict__ q = Q.q[j];
    const size_t n = (size_t)list[0] * (size_t)row_len;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const size_t r = i / (size_t)row_len, at = (size_t)list[1 + r] * (size_t)row_len + (i - r * (size_t)row_len);
        q[at] = quantize_feature(f[at], scale, zp);
    }
}

// ---------------------------------------------------------------------------------------------------------
//  launchers (called from kws_bank.cpp)
// ---------------------------------------------------------------------------------------------------------

// out.n members, all of activation-row width cp (16 or 64), each of the matrix-core shape (the caller checked kws_nn_uses_mfma)
int kws_launch_bank_nn_mfma(const KwsBankRec *recs, const KwsBankOut &out, int cp, const float *features, int n_clips, int grid_cap, hipStream_t stream)
{
    (void)hipGetLastError();      // the status returned below is this launch's, not a stale error of an earlier call
    if (n_clips <= 0 || out.n <= 0) return 0;
    if (out.n > KWS_BANK_MAX || (cp != 16 && cp != 64)) return (int)hipErrorInvalidValue;
    int grid = (n_clips + KWS_NN_WAVES - 1) / KWS_NN_WAVES;
    if (grid > grid_cap) grid = grid_cap;
    if (cp == 16)
        hipLaunchKernelGGL(kws_bank_nn_mfma_kernel<16>, dim3(grid, out.n), dim3(KWS_WAVE * KWS_NN_WAVES), 0, stream, recs, out, features, n_clips);
    else
        hipLaunchKernelGGL(kws_bank_nn_mfma_kernel<64>, dim3(grid, out.n), dim3(KWS_WAVE * KWS_NN_WAVES), 0, stream, recs, out, features, n_clips);
    return (int)hipGetLastError();
}

int kws_launch_bank_quantize(const float *features, size_t n, const KwsBankQuant &Q, hipStream_t stream)
{
    (void)hipGetLastError();
    if (n == 0 || Q.n <= 0) return 0;
    if (Q.n > KWS_BANK_MAX) return (int)hipErrorInvalidValue;
    size_t blocks = (n + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(kws_bank_quantize_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, features, n, Q);
    return (int)hipGetLastError();
}

// the routed forms: out.n / Q.n members with non-empty lists, n_longest the longest of them
int kws_launch_bank_nn_mfma_routed(const KwsBankRec *recs, const KwsBankOut &out, const KwsBankLists &lists, int cp, const float *features, int n_longest,
                                   int grid_cap, hipStream_t stream)
{
    (void)hipGetLastError();
    if (n_longest <= 0 || out.n <= 0) return 0;
    if (out.n > KWS_BANK_MAX || (cp != 16 && cp != 64)) return (int)hipErrorInvalidValue;
    int grid = (n_longest + KWS_NN_WAVES - 1) / KWS_NN_WAVES;
    if (grid > grid_cap) grid = grid_cap;
    if (cp == 16)
        hipLaunchKernelGGL(kws_bank_nn_mfma_routed_kernel<16>, dim3(grid, out.n), dim3(KWS_WAVE * KWS_NN_WAVES), 0, stream, recs, out, lists, features);
    else
        hipLaunchKernelGGL(kws_bank_nn_mfma_routed_kernel<64>, dim3(grid, out.n), dim3(KWS_WAVE * KWS_NN_WAVES), 0, stream, recs, out, lists, features);
    return (int)hipGetLastError();
}

int kws_launch_bank_quantize_routed(const float *features, int row_len, const KwsBankQuant &Q, const KwsBankLists &lists, int n_longest, hipStream_t stream)
{
    (void)hipGetLastError();
    if (n_longest <= 0 || row_len <= 0 || Q.n <= 0) return 0;
    if (Q.n > KWS_BANK_MAX) return (int)hipErrorInvalidValue;
    size_t blocks = ((size_t)n_longest * (size_t)row_len + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(kws_bank_quantize_routed_kernel, dim3((unsigned)blocks, Q.n), dim3(256), 0, stream, features, row_len, Q, lists);
    return (int)hipGetLastError();
}
