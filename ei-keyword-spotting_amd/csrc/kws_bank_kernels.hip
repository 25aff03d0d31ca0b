// kws_bank_kernels.hip -- the networks of a bank (kws_bank.cpp; contract in include/kws/kws.h) behind ONE float feature matrix:
// kws_bank_nn_mfma_kernel (every int8 member of the two-block matrix-core shape in one launch per activation-row width, quantising the
// features on load) and kws_bank_quantize_kernel (the int8 input tensors of the other int8 members in one pass over the matrix).  Each has
// two forms: the unrouted one, where every member takes every row, and the routed one (_routed_kernel), where each member takes its own
// list of rows.  The two forms of the matrix-core kernel share their set-up (bank_nn_stage) and the quantise-on-load of a feature row
// (bank_quantize_row), both in kws_bank_nn_dev.h, where the pool's kernel finds them too; each keeps its own loop over clips and its own
// LDS declarations, because one body behind both costs kws_bank_nn_mfma_kernel<64> four registers (profiles/bank_route_codeobj.md).
// The network itself is kws_nn_int8_dev.h's, unchanged: a member's scores are those of its own kws_nn_mfma_kernel launch bit for bit.
#include "kws_device.h"

#include "kws_nn_int8_dev.h"
#include "kws_bank.h"
#include "kws_bank_nn_dev.h"

// ---------------------------------------------------------------------------------------------------------
//  Grid (clip tiles, member): blockIdx.y picks the member's record in HBM (its plan and input quantisation; uniform over the
//  workgroup, so the plan is read through the scalar cache as kws_nn_mfma_kernel reads its by-value copy) and its score buffer in
//  the launch arguments.  The workgroup stages that member's head and ADD tables once; each wave then takes clips: the clip's float
//  feature row is read once and quantised straight into the act1 rows, and nn_mfma_clip does the rest.  LDS and registers: those of
//  kws_nn_mfma_kernel<CP>.
//    unrouted   a wave takes clips blockIdx.x * KWS_NN_WAVES + wave, ... of 0 .. n_clips - 1
//    routed     the same grid, sized by the longest list of the launch; slot blockIdx.y walks lists.list[blockIdx.y] -- [0] = how many,
//               then the clips, ascending -- instead: a wave's position in the list is uniform, so the clip index is one scalar load
// ---------------------------------------------------------------------------------------------------------
template <int CP>
__global__ __launch_bounds__(KWS_WAVE * KWS_NN_WAVES) void kws_bank_nn_mfma_kernel(const KwsBankRec *__restrict__ recs, KwsBankOut out,
                                                                                   const float *__restrict__ features, int n_clips)
{
    KWS_BANK_NN_LDS(CP);
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));    // uniform: per-wave addresses stay in scalar registers
    const int slot = (int)blockIdx.y;
    const KwsBankRec &R = recs[out.rec[slot]];
    const KwsNnPlan &N = R.N;
    float *__restrict__ scores = out.scores[slot];
    const KwsConvBlock &k1 = N.blk[0];
    int8_t *act1 = s_act1[wave], *act2 = s_act2[wave];
    NnMfmaCtx<CP> ctx;
    const NnHeadTab head = bank_nn_stage<CP>(N, s_head, s_lut1, s_lut2, act1, act2, ctx, lane);
    const int F = N.n_features, in_c = k1.in_c, pad_left = k1.pad_left;
    const float in_scale = R.in_scale;
    const int in_zp = R.in_zp;
    const unsigned inv_c = (1u << 20) / (unsigned)in_c + 1u;
    const bool quads = (in_c & 3) == 0 && ((uintptr_t)features & 15) == 0;
    const NnTaps taps = { nullptr, 0, nullptr, nullptr, nullptr, nullptr };
    for (int clip = blockIdx.x * KWS_NN_WAVES + wave; clip < n_clips; clip += gridDim.x * KWS_NN_WAVES) {
        bank_quantize_row<CP>(features + (size_t)clip * F, act1, F, in_c, pad_left, inv_c, quads, in_scale, in_zp, lane);
        WAVE_SYNC();
        nn_mfma_clip<CP>(ctx, N, head, act1, act2, s_vec[wave], s_lut1, s_lut2, lane, clip, scores, taps);
    }
}

template <int CP>
__global__ __launch_bounds__(KWS_WAVE * KWS_NN_WAVES) void kws_bank_nn_mfma_routed_kernel(const KwsBankRec *__restrict__ recs, KwsBankOut out, KwsBankLists lists,
                                                                                          const float *__restrict__ features)
{
    KWS_BANK_NN_LDS(CP);
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int slot = (int)blockIdx.y;
    const KwsBankRec &R = recs[out.rec[slot]];
    const KwsNnPlan &N = R.N;
    float *__restrict__ scores = out.scores[slot];
    const KwsConvBlock &k1 = N.blk[0];
    int8_t *act1 = s_act1[wave], *act2 = s_act2[wave];
    NnMfmaCtx<CP> ctx;
    const NnHeadTab head = bank_nn_stage<CP>(N, s_head, s_lut1, s_lut2, act1, act2, ctx, lane);
    const int F = N.n_features, in_c = k1.in_c, pad_left = k1.pad_left;
    const float in_scale = R.in_scale;
    const int in_zp = R.in_zp;
    const unsigned inv_c = (1u << 20) / (unsigned)in_c + 1u;
    const bool quads = (in_c & 3) == 0 && ((uintptr_t)features & 15) == 0;
    const NnTaps taps = { nullptr, 0, nullptr, nullptr, nullptr, nullptr };
    const int *__restrict__ list = lists.list[slot];
    const int n_list = list[0];
    for (int ci = blockIdx.x * KWS_NN_WAVES + wave; ci < n_list; ci += gridDim.x * KWS_NN_WAVES) {
        const int clip = __builtin_amdgcn_readfirstlane(list[1 + ci]);
        bank_quantize_row<CP>(features + (size_t)clip * F, act1, F, in_c, pad_left, inv_c, quads, in_scale, in_zp, lane);
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
//  launchers (called from kws_bank.cpp).  lists == NULL: the unrouted form over rows 0 .. n_rows - 1; otherwise the routed form, the
//  members having non-empty lists and n_rows being the longest of them.  n_rows sizes the grid either way.
// ---------------------------------------------------------------------------------------------------------

// out.n members, all of activation-row width cp (16 or 64), each of the matrix-core shape (the caller checked kws_nn_uses_mfma)
int kws_launch_bank_nn_mfma(const KwsBankRec *recs, const KwsBankOut &out, const KwsBankLists *lists, int cp, const float *features, int n_rows, int grid_cap,
                            hipStream_t stream)
{
    (void)hipGetLastError();      // the status returned below is this launch's, not a stale error of an earlier call
    if (n_rows <= 0 || out.n <= 0) return 0;
    if (out.n > KWS_BANK_MAX || (cp != 16 && cp != 64)) return (int)hipErrorInvalidValue;
    int grid = (n_rows + KWS_NN_WAVES - 1) / KWS_NN_WAVES;
    if (grid > grid_cap) grid = grid_cap;
    const dim3 blocks(grid, out.n), threads(KWS_WAVE * KWS_NN_WAVES);
    if (!lists && cp == 16) hipLaunchKernelGGL(kws_bank_nn_mfma_kernel<16>, blocks, threads, 0, stream, recs, out, features, n_rows);
    else if (!lists) hipLaunchKernelGGL(kws_bank_nn_mfma_kernel<64>, blocks, threads, 0, stream, recs, out, features, n_rows);
    else if (cp == 16) hipLaunchKernelGGL(kws_bank_nn_mfma_routed_kernel<16>, blocks, threads, 0, stream, recs, out, *lists, features);
    else hipLaunchKernelGGL(kws_bank_nn_mfma_routed_kernel<64>, blocks, threads, 0, stream, recs, out, *lists, features);
    return (int)hipGetLastError();
}

// row_len: values per feature row; routed, member slot j's tensor is written only at its listed rows
int kws_launch_bank_quantize(const float *features, int n_rows, int row_len, const KwsBankQuant &Q, const KwsBankLists *lists, hipStream_t stream)
{
    (void)hipGetLastError();
    if (n_rows <= 0 || row_len <= 0 || Q.n <= 0) return 0;
    if (Q.n > KWS_BANK_MAX) return (int)hipErrorInvalidValue;
    const size_t n = (size_t)n_rows * (size_t)row_len;
    size_t blocks = (n + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    if (lists) hipLaunchKernelGGL(kws_bank_quantize_routed_kernel, dim3((unsigned)blocks, Q.n), dim3(256), 0, stream, features, row_len, Q, *lists);
    else hipLaunchKernelGGL(kws_bank_quantize_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, features, n, Q);
    return (int)hipGetLastError();
}
