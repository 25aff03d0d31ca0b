// kws_pool_kernels.hip -- the kernels of a pool (kws_pool.cpp; contract in include/kws/kws.h): hundreds of int8 members of the two-block
// matrix-core shape behind ONE float feature matrix, each row scored by the one member it names.
//   kws_pool_nn_mfma_kernel<CP>   every member's network in one launch over a flat table of work items in HBM: one workgroup per item
//   kws_pool_maf_live_kernel      continuous mode's filter of a live push on rows of `stride` floats, the member being the stream's assignment
//   kws_pool_maf_scan_kernel      the same for a recording scan: a fresh filter per recording, the member being the recording's
// The network kernel is built from the bank kernel's pieces, unchanged (kws_bank_nn_dev.h: bank_nn_stage, bank_quantize_row; kws_nn_int8_dev.h:
// nn_mfma_clip), so a row's scores are those of its member's own kws_nn_mfma_kernel launch bit for bit.  nn_mfma_clip stores a clip's scores
// at scores[clip * fc_out + lane] and reads `clip` otherwise only for the parity taps, which a pool call does not request: with clip = 0 and
// the base pointer scores + row * stride it writes the row's first fc_out columns at any stride, and nothing beyond them.
#include "kws_device.h"
#include "kws_window_kernels.h"

#include "kws_nn_int8_dev.h"
#include "kws_pool.h"
#include "kws_bank_nn_dev.h"

#include "../../include/kws/ei_compat.h"

#define KWS_POOL_TAPS (EI_CLASSIFIER_SLICES_PER_MODEL_WINDOW >> 1)

int kws_pool_nn_fits(const KwsNnPlan &N) { return nn_fits_mfma(N) ? 1 : 0; }

// ---------------------------------------------------------------------------------------------------------
//  Grid (items): blockIdx.x picks the work item -- (member, first position of the row list, count) -- from the table in HBM; the item
//  is uniform over the workgroup, so it and the member's plan are read through the scalar cache, as the bank kernel reads its record.
//  The workgroup stages that member's head and ADD tables once; wave w then walks the list positions first + w, first + w + KWS_NN_WAVES,
//  ...: the row index is one scalar load, the row's float features are read once and quantised straight into the act1 rows, and
//  nn_mfma_clip does the rest.  LDS and registers: those of kws_bank_nn_mfma_routed_kernel<CP> (profiles/pool_codeobj.md).
// ---------------------------------------------------------------------------------------------------------
template <int CP>
__global__ __launch_bounds__(KWS_WAVE * KWS_NN_WAVES) void kws_pool_nn_mfma_kernel(const KwsBankRec *__restrict__ recs, const KwsPoolItem *__restrict__ items,
                                                                                   const int *__restrict__ rows, const float *__restrict__ features,
                                                                                   float *__restrict__ scores, int stride)
{
    KWS_BANK_NN_LDS(CP);
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const KwsPoolItem item = items[blockIdx.x];
    const int member = __builtin_amdgcn_readfirstlane(item.member), first = __builtin_amdgcn_readfirstlane(item.first),
              count = __builtin_amdgcn_readfirstlane(item.count);
    const KwsBankRec &R = recs[member];
    const KwsNnPlan &N = R.N;
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
    const int *__restrict__ list = rows + first;
    for (int ci = wave; ci < count; ci += KWS_NN_WAVES) {
        const int row = __builtin_amdgcn_readfirstlane(list[ci]);
        bank_quantize_row<CP>(features + (size_t)row * F, act1, F, in_c, pad_left, inv_c, quads, in_scale, in_zp, lane);
        WAVE_SYNC();
        nn_mfma_clip<CP>(ctx, N, head, act1, act2, s_vec[wave], s_lut1, s_lut2, lane, 0, scores + (size_t)row * stride, taps);
    }
}

// ---------------------------------------------------------------------------------------------------------
//  The live moving average: thread t = a * stride + l is entry a, column l.  The member is the stream's assignment; the thread ends before
//  any read of a row or of filter state if the stream is unassigned or the column is at or above the member's label count.  Otherwise it is
//  bank_maf<true, ...>'s arithmetic (kws_bank_windows_kernels.hip), operation for operation: the w0 / k_full rule, the index as the window
//  count mod taps, subtract the oldest tap from the running sum, add the new value, store it as the tap, out = sum / (float)taps, and no
//  store of the state for a stream the push finishes -- on rows of `stride` floats and state at ((stream * stride) + l) * (taps + 1).
// ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void kws_pool_maf_live_kernel(const float *__restrict__ raw, float *__restrict__ scores, KwsLiveMeta m, int n, int stride,
                                                               const uint32_t *__restrict__ assign, const int *__restrict__ labels, int k_full,
                                                               float *__restrict__ maf)
{
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (long long)n * stride) return;
    const int a = (int)(t / stride);
    const int l = (int)(t - (long long)a * stride);
    const long long stream = m.stream[a];
    const uint32_t member = assign[stream];
    if (member == KWS_POOL_NONE || l >= labels[member]) return;
    const long long g0 = m.wbase[a], g1 = m.wbase[a + 1];
    if (g0 == g1) return;
    const long long w0 = m.k0[a] > k_full ? m.k0[a] - k_full : 0;
    float *st = maf + ((size_t)stream * stride + l) * (KWS_POOL_TAPS + 1);
    const bool store = !m.fin[a];
    float buf[KWS_POOL_TAPS];
    float rs = 0.0f;
#pragma unroll
    for (int j = 0; j < KWS_POOL_TAPS; ++j) buf[j] = w0 ? st[j] : 0.0f;
    if (w0) rs = st[KWS_POOL_TAPS];
    int idx = (int)(w0 % KWS_POOL_TAPS);
    for (long long g = g0; g < g1; ++g) {
        const float v = raw[(size_t)g * stride + l];
        rs -= buf[idx];
        rs += v;
        buf[idx] = v;
        scores[(size_t)g * stride + l] = rs / (float)KWS_POOL_TAPS;
        if (++idx >= KWS_POOL_TAPS) idx = 0;
    }
    if (!store) return;
#pragma unroll
    for (int j = 0; j < KWS_POOL_TAPS; ++j) st[j] = buf[j];
    st[KWS_POOL_TAPS] = rs;
}

// ---------------------------------------------------------------------------------------------------------
//  The scan's moving average: thread t = a * stride + l is recording a (of the n that have windows), column l.  The member is the
//  recording's, from the table uploaded with the call; the thread ends before any read of a row if the recording names nobody or the column
//  is at or above the member's label count.  Otherwise it is kws_scan_maf_kernel's arithmetic (kws_scan_kernels.hip), operation for
//  operation: fresh taps and a running sum of zero, the index from 0, subtract the oldest tap, add the new value, store it as the tap,
//  out = sum / (float)taps -- on rows of `stride` floats from wbase[a] to wbase[a + 1].  raw and scores may be the same buffer (a scan
//  without raw_scores filters in place), so neither is __restrict__.  A body of its own: kws_pool_maf_live_kernel stays what it is.
// ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void kws_pool_maf_scan_kernel(const float *raw, float *scores, const long long *__restrict__ wbase, int n, int stride,
                                                               const uint32_t *__restrict__ members, const int *__restrict__ labels)
{
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (long long)n * stride) return;
    const int a = (int)(t / stride);
    const int l = (int)(t - (long long)a * stride);
    const uint32_t member = members[a];
    if (member == KWS_POOL_NONE || l >= labels[member]) return;
    float buf[KWS_POOL_TAPS];
#pragma unroll
    for (int j = 0; j < KWS_POOL_TAPS; ++j) buf[j] = 0.0f;
    float rs = 0.0f;
    int idx = 0;
    for (long long g = wbase[a]; g < wbase[a + 1]; ++g) {
        const float v = raw[(size_t)g * stride + l];
        rs -= buf[idx];
        rs += v;
        buf[idx] = v;
        scores[(size_t)g * stride + l] = rs / (float)KWS_POOL_TAPS;
        if (++idx >= KWS_POOL_TAPS) idx = 0;
    }
}

// ---------------------------------------------------------------------------------------------------------
//  launchers (called from kws_pool.cpp)
// ---------------------------------------------------------------------------------------------------------
int kws_launch_pool_nn_mfma(const KwsBankRec *recs, const KwsPoolItem *items, int n_items, const int *rows, int cp, const float *features, float *scores, int stride,
                            hipStream_t stream)
{
    (void)hipGetLastError();      // the status returned below is this launch's, not a stale error of an earlier call
    if (n_items <= 0) return 0;
    if (cp != 16 && cp != 64) return (int)hipErrorInvalidValue;
    const dim3 blocks(n_items), threads(KWS_WAVE * KWS_NN_WAVES);
    if (cp == 16) hipLaunchKernelGGL(kws_pool_nn_mfma_kernel<16>, blocks, threads, 0, stream, recs, items, rows, features, scores, stride);
    else hipLaunchKernelGGL(kws_pool_nn_mfma_kernel<64>, blocks, threads, 0, stream, recs, items, rows, features, scores, stride);
    return (int)hipGetLastError();
}

int kws_launch_pool_maf_live(const float *raw, float *scores, const long long *meta, int n_act, int stride, const uint32_t *assign, const int *labels, int k_full,
                             float *maf, hipStream_t stream)
{
    (void)hipGetLastError();
    const long long n = (long long)n_act * stride;
    if (n <= 0) return 0;
    hipLaunchKernelGGL(kws_pool_maf_live_kernel, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, stream, raw, scores, live_meta(meta, n_act), n_act, stride, assign, labels,
                       k_full, maf);
    return (int)hipGetLastError();
}

int kws_launch_pool_maf_scan(const float *raw, float *scores, const long long *wbase, int n_rec, int stride, const uint32_t *member, const int *labels,
                             hipStream_t stream)
{
    (void)hipGetLastError();
    const long long n = (long long)n_rec * stride;
    if (n <= 0) return 0;
    hipLaunchKernelGGL(kws_pool_maf_scan_kernel, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, stream, raw, scores, wbase, n_rec, stride, member, labels);
    return (int)hipGetLastError();
}
