// kws_nn_f32.hip -- kws_nn_f32_kernel<MAXT, TRUNK, SD> (kws_nn_f32_generic.h) and kws_dense_f32_kernel: float32 graphs (the reference's float
// TFLite-Micro kernels replayed).
#include <algorithm>

#include "kws_device.h"
#include "kws_nn2d.h"
#include "kws_nnres.h"

// ---------------------------------------------------------------------------------------------------------
//  Kernel 2f: float32 models.  One wave per clip.  Every accumulation replays the reference's sequential
//  `total += input * filter` order (tap outer, channel inner; product and sum rounded separately -- the build has
//  -ffp-contract=off), so everything up to the logits is bit-identical to the float TFLite-Micro kernels; only softmax's
//  expf is the device's.  Zero-padded activation rows stand in for the reference's skipped out-of-image taps: for a FINITE
//  weight they add an exact 0 (0*w = +-0, and total + (+-0) == total for every total the chain can hold, +0 included: a
//  chain starts at +0 and +0 + -0 = +0).  PRECONDITION: every conv / depthwise weight is finite -- 0 * inf = NaN where the
//  reference never touches the tap; build_nn_plan_f32 refuses a model with a non-finite weight (kws_plan.cpp).
//
//  The multiply-adds of a clip are order-constrained only WITHIN one output's chain, so a lane runs TB x OB chains (TB
//  consecutive time steps x OB consecutive output channels) side by side: per chain step it reads TB activations and one
//  OB-wide weight vector from LDS for TB*OB independent mul+add pairs.  The plan picks (TB, OB) per conv block so that the
//  work items fill the 64 lanes (shipped shape: conv1 49x30 -> 7x4, 56 lanes; conv2 7x10 -> 1x2, 35 lanes); a lane that
//  owns exactly one pooling window max-pools in registers, an un-pooled block writes straight into the next image.
//  LDS: per workgroup the weights of every block transposed to [tap*in_c + c][out_c padded to 4]; per wave the ping-pong
//  input images A / B (zero-padded rows), Y only for blocks whose pooling cannot happen in registers, and 128 floats for
//  the FULLY_CONNECTED input / logits.  The plan is read from device memory (nnf_layout() is shared with the host).
//  LDS locations are carried as offsets from the extern __shared__ base (pointers kept in arrays degrade to flat loads); the
//  next clip's feature vector is requested after block 0 and placed at the next iteration's top (256-register build).
// ---------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float act_clamp(float x, float lo, float hi)   // ActivationFunctionWithMinMax
{
    const float a = x < lo ? lo : x;
    return hi < a ? hi : a;
}

// how a block's outputs leave the conv: pooled in registers (fused_pool), written straight to the next image (no pooling
// node), or staged in Y for a separate pooling pass
__host__ __device__ __forceinline__ bool nnf_direct(const KwsConvBlockF32 &k) { return k.pool == 1; }
__host__ __device__ __forceinline__ bool nnf_staged(const KwsConvBlockF32 &k) { return !k.fused_pool && !nnf_direct(k); }
__host__ __device__ __forceinline__ int nnf_ntb_of(const KwsConvBlockF32 &k) { return k.fused_pool ? k.pool_w : (k.out_w + k.tb - 1) / k.tb; }
__host__ __device__ __forceinline__ int nnf_rows_of(const KwsConvBlockF32 &k)       // rows of the zero-padded input image
{
    // rows the blocked walk touches (k.tb is final): output t, tap j reads row t * stride + j * dilation, and the last, ragged block of tb time steps is
    // computed whole (stride 1, dilation 1: ntb * tb + taps - 1 as ever)
    const int a = k.pad_left + k.in_w, b = (nnf_ntb_of(k) * k.tb - 1) * k.stride + (k.taps - 1) * k.dilation + 1;
    return a > b ? a : b;
}
// x / d for an item index: the plan's reciprocal where it is exact (x d < 2^20), a real division (~35 vector instructions) elsewhere
__device__ __forceinline__ int nnf_div(int x, int d, unsigned inv20) { return inv20 ? (int)(((unsigned)x * inv20) >> 20) : x / d; }
// ... as the plan holds them (kws_nn_f32_pick_blocking sets both with the blocking)
__host__ __device__ __forceinline__ int nnf_ntb(const KwsConvBlockF32 &k) { return k.ntb; }
__host__ __device__ __forceinline__ int nnf_rows(const KwsConvBlockF32 &k) { return k.rows; }
__host__ __device__ __forceinline__ int nnf_ocp(const KwsConvBlockF32 &k) { return (k.out_c + 3) & ~3; }
// LDS position of weight (step j, output channel oc) of a conv block: [j][oc] (a lane reads OB consecutive channels of one
// step) for register-blocked blocks; [oc block][j][OB] for one-time-step blocks, whose lanes stream their own weights
__device__ __forceinline__ int nnf_w_index(const KwsConvBlockF32 &k, int J, int j, int oc)
{
    if (k.depthwise || k.tb != 1) return j * nnf_ocp(k) + oc;
    return ((oc / k.ob) * J + j) * k.ob + (oc % k.ob);
}

// where a block's (pooled) output goes: the next block's zero-padded input image, or the FULLY_CONNECTED input vector
struct NnfDst { float *p; int row0, stride; };

// CONV_2D float: a lane owns TB consecutive time steps x OB consecutive output channels.  SD chooses the loop nest of the chains (stride 1: one contiguous
// run per chain; strided / dilated: tap by tap); the item split in front of it and the epilogue behind it are the same.
template <int TB, int OB, bool VEC4, bool SD>
__device__ __forceinline__ void nnf_conv(const KwsConvBlockF32 &k, const float *__restrict__ x, const float *__restrict__ wt,
                                         float *__restrict__ y, const NnfDst &dst, int lane)
{
    const int J = k.taps * k.in_c, ocp = nnf_ocp(k);
    const int n_ob = (k.out_c + OB - 1) / OB, n_tb = nnf_ntb(k);
    const bool direct = nnf_direct(k);
    const int xs = (SD ? k.stride : 1) * k.in_c, ts = (SD ? k.dilation : 1) * k.in_c;      // floats between the rows of two consecutive outputs / taps
    for (int item = lane; item < n_tb * n_ob; item += 64) {
        const int tb = nnf_div(item, n_ob, k.inv_item20), ob = item - tb * n_ob;
        const int t0 = tb * TB, oc0 = ob * OB;
        float acc[TB][OB];
#pragma unroll
        for (int i = 0; i < TB; ++i)
#pragma unroll
            for (int o = 0; o < OB; ++o) acc[i][o] = 0.0f;
        if constexpr (SD) {
            // strided / dilated: output t, tap j reads image row t * stride + j * dilation, so a chain's activations are no longer one
            // contiguous run of taps * in_c floats: the steps run tap by tap, channel by channel inside a tap -- the reference's order, products and sums
            // rounded separately -- and the zero rows of the padded image stand in for the skipped taps as ever.  Weights keep their LDS layouts.
            const float *xp = x + t0 * xs;
            // step j's OB weights: [j][oc] for register-blocked blocks, [oc block][j][OB] for one-time-step blocks (nnf_w_index)
            const float *wp = TB == 1 ? wt + (size_t)ob * J * OB : wt + oc0;
            const int wstep = TB == 1 ? OB : ocp;
            auto load_w = [&](int j, float (&w)[OB]) {
                if constexpr (OB == 4 && TB != 1) { const float4 v = *(const float4 *)(wp + j * wstep); w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w; }
                else if constexpr (OB == 2 && TB != 1) { const float2 v = *(const float2 *)(wp + j * wstep); w[0] = v.x; w[1] = v.y; }
                else {
#pragma unroll
                    for (int o = 0; o < OB; ++o) w[o] = wp[j * wstep + o];
                }
            };
            if (VEC4 && (k.in_c & 3) == 0) {
                // rows are 16-byte aligned: one 16-byte read per time row brings the activations of 4 consecutive steps of a tap
                for (int tap = 0; tap < k.taps; ++tap) {
                    const float *xt = xp + tap * ts;
                    for (int c = 0; c < k.in_c; c += 4) {
                        float4 xv[TB];
                        float w[4][OB];
#pragma unroll
                        for (int i = 0; i < TB; ++i) xv[i] = *(const float4 *)(xt + i * xs + c);
#pragma unroll
                        for (int u = 0; u < 4; ++u) load_w(tap * k.in_c + c + u, w[u]);
#pragma unroll
                        for (int u = 0; u < 4; ++u) {                  // chain order: channels c, c+1, c+2, c+3
#pragma unroll
                            for (int i = 0; i < TB; ++i) {
                                const float xs_ = u == 0 ? xv[i].x : u == 1 ? xv[i].y : u == 2 ? xv[i].z : xv[i].w;
#pragma unroll
                                for (int o = 0; o < OB; ++o) {
                                    const float prod = xs_ * w[u][o];
                                    acc[i][o] += prod;
                                }
                            }
                        }
                    }
                }
            } else {
                for (int tap = 0; tap < k.taps; ++tap) {
                    const float *xt = xp + tap * ts;
                    for (int c = 0; c < k.in_c; ++c) {
                        float w[OB], xv[TB];
                        load_w(tap * k.in_c + c, w);
#pragma unroll
                        for (int i = 0; i < TB; ++i) xv[i] = xt[i * xs + c];
#pragma unroll
                        for (int i = 0; i < TB; ++i) {
#pragma unroll
                            for (int o = 0; o < OB; ++o) {
                                const float prod = xv[i] * w[o];
                                acc[i][o] += prod;
                            }
                        }
                    }
                }
            }
        } else {
            const float *xp = x + t0 * k.in_c;          // rows are contiguous: x[(t+tap)*in_c + c] == x[t*in_c + (tap*in_c + c)]
            const float *wp = wt + oc0;
            // software pipeline: the TB activations and the OB-wide weight vector of step j+1 are in flight while step j's
            // TB*OB multiply-adds issue (LDS latency would otherwise be exposed once per step at 2 waves per SIMD)
            float wn[OB], xn[TB];
            auto load_w = [&](int j, float (&w)[OB]) {
                if constexpr (OB == 4) { const float4 v = *(const float4 *)(wp + j * ocp); w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w; }
                else if constexpr (OB == 2) { const float2 v = *(const float2 *)(wp + j * ocp); w[0] = v.x; w[1] = v.y; }
                else w[0] = wp[j * ocp];
            };
            if constexpr (TB == 1) {
                // one time step per lane (small blocks): a chain step is a single multiply-add per output channel, so issue
                // slots decide.  The weights of such a block sit in LDS as [oc block][step][OB] (nnf_w_index), i.e. a lane's
                // weight stream is contiguous: 8 steps' operands are 16 * OB / 4 + 4 reads at immediate offsets from two running
                // pointers, full batches run without clamps or predicates, the J % 8 last steps one by one.  (No double
                // buffering: the rotating copies cost more issue slots than the exposed round trip, which the SIMD's other
                // wave -- usually inside a register-blocked block -- fills.)
                typedef float f2v __attribute__((ext_vector_type(2)));
                constexpr int U = 8, NV = (OB + 1) / 2;
                const float *wq = wt + (size_t)ob * J * OB;
                const int Jm = J & ~(U - 1);
                f2v a2[NV];
#pragma unroll
                for (int v = 0; v < NV; ++v) a2[v] = (f2v){ 0.0f, 0.0f };
                auto step1 = [&](const float *wj, float xs_) {        // products and sums rounded separately (-ffp-contract=off)
                    if constexpr (OB == 1) { const float prod = xs_ * wj[0]; a2[0].x += prod; }
                    else {
#pragma unroll
                        for (int v = 0; v < NV; ++v) {
                            const f2v wv = { wj[2 * v], wj[2 * v + 1] };
                            const f2v prod = wv * xs_;
                            a2[v] += prod;
                        }
                    }
                };
                for (int j0 = 0; j0 < Jm; j0 += U) {
                    float w[U * OB], xs_[U];
#pragma unroll
                    for (int i = 0; i < U * OB; ++i) w[i] = wq[j0 * OB + i];
#pragma unroll
                    for (int u = 0; u < U; ++u) xs_[u] = xp[j0 + u];
#pragma unroll
                    for (int u = 0; u < U; ++u) step1(w + u * OB, xs_[u]);
                }
                for (int j = Jm; j < J; ++j) {
                    float w[OB];
#pragma unroll
                    for (int o = 0; o < OB; ++o) w[o] = wq[j * OB + o];
                    step1(w, xp[j]);
                }
#pragma unroll
                for (int o = 0; o < OB; ++o) acc[0][o] = (o & 1) ? a2[o >> 1].y : a2[o >> 1].x;
            } else if (VEC4 && (k.in_c & 3) == 0) {
                // channel counts that are multiples of 4 (rows 16-byte aligned): FOUR chain steps per batch -- one 16-byte read
                // per time row brings the activations of 4 consecutive steps, the batch after next is in flight meanwhile
                // (TB + 4 LDS instructions per 4 steps instead of 4 * (TB + 1)); needs the 256-register build of the kernel
                float4 xq[TB];
                float wq[4][OB];
                auto load_batch = [&](int j) {
#pragma unroll
                    for (int u = 0; u < 4; ++u) load_w(j + u, wq[u]);
#pragma unroll
                    for (int i = 0; i < TB; ++i) xq[i] = *(const float4 *)(xp + i * k.in_c + j);
                };
                load_batch(0);
                for (int j = 0; j < J; j += 4) {
                    float4 xv[TB];
                    float w[4][OB];
#pragma unroll
                    for (int i = 0; i < TB; ++i) xv[i] = xq[i];
#pragma unroll
                    for (int u = 0; u < 4; ++u)
#pragma unroll
                        for (int o = 0; o < OB; ++o) w[u][o] = wq[u][o];
                    load_batch(min(j + 4, J - 4));
#pragma unroll
                    for (int u = 0; u < 4; ++u) {                      // chain order: steps j, j+1, j+2, j+3
#pragma unroll
                        for (int i = 0; i < TB; ++i) {
                            const float xs_ = u == 0 ? xv[i].x : u == 1 ? xv[i].y : u == 2 ? xv[i].z : xv[i].w;
#pragma unroll
                            for (int o = 0; o < OB; ++o) {
                                const float prod = xs_ * w[u][o];
                                acc[i][o] += prod;
                            }
                        }
                    }
                }
            } else {
                load_w(0, wn);
#pragma unroll
                for (int i = 0; i < TB; ++i) xn[i] = xp[i * k.in_c];
                for (int j = 0; j < J; ++j) {
                    float w[OB], xv[TB];
#pragma unroll
                    for (int o = 0; o < OB; ++o) w[o] = wn[o];
#pragma unroll
                    for (int i = 0; i < TB; ++i) xv[i] = xn[i];
                    const int jn = min(j + 1, J - 1);
                    load_w(jn, wn);
#pragma unroll
                    for (int i = 0; i < TB; ++i) xn[i] = xp[i * k.in_c + jn];
#pragma unroll
                    for (int i = 0; i < TB; ++i) {
#pragma unroll
                        for (int o = 0; o < OB; ++o) {
                            const float prod = xv[i] * w[o];
                            acc[i][o] += prod;
                        }
                    }
                }
            }
        }
#pragma unroll
        for (int o = 0; o < OB; ++o) {
            const int oc = oc0 + o;
            if (oc >= k.out_c) continue;
            const float bv = k.bias[oc], av = k.addc[oc];
            float mx = -FLT_MAX;
#pragma unroll
            for (int i = 0; i < TB; ++i) {
                if (t0 + i < k.out_w) {
                    float v = act_clamp(acc[i][o] + bv, k.conv_min, k.conv_max);
                    if (k.has_add) v = act_clamp(v + av, k.add_min, k.add_max);
                    if (k.fused_pool) mx = mx < v ? v : mx;             // MAX_POOL_2D: std::max(max, v), window order
                    else if (direct) dst.p[(dst.row0 + t0 + i) * dst.stride + oc] = v;
                    else y[(t0 + i) * k.out_c + oc] = v;
                }
            }
            if (k.fused_pool) dst.p[(dst.row0 + tb) * dst.stride + oc] = act_clamp(mx, k.pool_min, k.pool_max);
        }
    }
}

// DEPTHWISE_CONV_2D float (reference/depthwiseconv_float.h:25-97): the chain of output (t, oc) runs over the taps of input
// channel oc / depth_mult only.  A lane owns TB consecutive time steps of one output channel.  SD: the strided / dilated form (as in nnf_conv);
// without it both row steps are in_c, as they always were.
template <int TB, bool SD>
__device__ __forceinline__ void nnf_dwconv(const KwsConvBlockF32 &k, const float *__restrict__ x, const float *__restrict__ wt,
                                           float *__restrict__ y, const NnfDst &dst, int lane)
{
    const int ocp = nnf_ocp(k), n_tb = nnf_ntb(k);
    const bool direct = nnf_direct(k);
    const int xs = (SD ? k.stride : 1) * k.in_c, ts = (SD ? k.dilation : 1) * k.in_c;      // floats between the rows of two consecutive outputs / taps
    for (int item = lane; item < n_tb * k.out_c; item += 64) {
        const int tb = nnf_div(item, k.out_c, k.inv_outc20), oc = item - tb * k.out_c;
        const int t0 = tb * TB;
        const float *xp = x + t0 * xs + (k.depth_mult == 1 ? oc : oc / k.depth_mult);
        float acc[TB];
#pragma unroll
        for (int i = 0; i < TB; ++i) acc[i] = 0.0f;
        for (int tap = 0; tap < k.taps; ++tap) {
            const float w = wt[tap * ocp + oc];
#pragma unroll
            for (int i = 0; i < TB; ++i) {
                const float prod = xp[i * xs + tap * ts] * w;
                acc[i] += prod;
            }
        }
        const float bv = k.bias[oc], av = k.addc[oc];
        float mx = -FLT_MAX;
#pragma unroll
        for (int i = 0; i < TB; ++i) {
            if (t0 + i < k.out_w) {
                float v = act_clamp(acc[i] + bv, k.conv_min, k.conv_max);
                if (k.has_add) v = act_clamp(v + av, k.add_min, k.add_max);
                if (k.fused_pool) mx = mx < v ? v : mx;
                else if (direct) dst.p[(dst.row0 + t0 + i) * dst.stride + oc] = v;
                else y[(t0 + i) * k.out_c + oc] = v;
            }
        }
        if (k.fused_pool) dst.p[(dst.row0 + tb) * dst.stride + oc] = act_clamp(mx, k.pool_min, k.pool_max);
    }
}

// a block's convolution at its blocking: depthwise or not, OB output channels per lane, stride-1 or strided form
template <int TB, bool VEC4, bool SD>
__device__ __forceinline__ void nnf_conv_ob(const KwsConvBlockF32 &k, const float *x, const float *wt, float *y, const NnfDst &dst, int lane)
{
    if (k.depthwise) nnf_dwconv<TB, SD>(k, x, wt, y, dst, lane);
    else if (k.ob == 4) nnf_conv<TB, 4, VEC4, SD>(k, x, wt, y, dst, lane);
    else if (k.ob == 2) nnf_conv<TB, 2, VEC4, SD>(k, x, wt, y, dst, lane);
    else nnf_conv<TB, 1, VEC4, SD>(k, x, wt, y, dst, lane);
}

// LDS layout shared by host and device: weights of every block, then per wave the ping-pong input images A (even blocks) and
// B (odd blocks), the un-pooled conv output Y (only when some block cannot pool in registers) and 128 floats for FC/softmax
struct NnfLayout { int w_floats, a_floats, b_floats, y_floats, fc_floats, vec_floats; };
__host__ __device__ __forceinline__ NnfLayout nnf_layout(const KwsNnPlanF32 &N)
{
    NnfLayout L = { 0, 0, 0, 0, 0, 0 };
    for (int b = 0; b < N.n_blocks; ++b) {
        const KwsConvBlockF32 &k = N.blk[b];
        L.w_floats += (k.depthwise ? k.taps : k.taps * k.in_c) * nnf_ocp(k);
        const int img = nnf_rows(k) * k.in_c;
        if (b & 1) L.b_floats = img > L.b_floats ? img : L.b_floats;
        else L.a_floats = img > L.a_floats ? img : L.a_floats;
        if (nnf_staged(k)) { const int yf = k.out_w * k.out_c; L.y_floats = yf > L.y_floats ? yf : L.y_floats; }
    }
    L.a_floats = (L.a_floats + 3) & ~3; L.b_floats = (L.b_floats + 3) & ~3; L.y_floats = (L.y_floats + 3) & ~3;
    // FULLY_CONNECTED weights + bias, shared by the workgroup (a global read per chain step would be an L2 round trip each);
    // per wave: the FC input vector (the last block's pooled output, also reused for the exponentials) + 64 floats of logits
    L.fc_floats = (N.fc_out * N.fc_in + N.fc_out + 3) & ~3;
    L.vec_floats = (((N.fc_in > 64 ? N.fc_in : 64) + 3) & ~3) + 64;
    return L;
}

#include "kws_nn_f32_generic.h"

// ---------------------------------------------------------------------------------------------------------
//  kws_dense_f32_kernel: the dense stack of a float32 graph (1 .. 4 FULLY_CONNECTED, fully_connected.h:26-60, then SOFTMAX, softmax.h:31-63).
//  Every output is ONE chain -- total += x[d] * w[o][d] for d = 0 .. K - 1, product and sum rounded separately, then + bias, then the clamp --
//  and only the order inside a chain is fixed.  So a lane owns a CLIP (a workgroup 64 of them) and the workgroup's waves share a layer's units,
//  KWS_DENSEF_UB chains per lane side by side: a weight is the same for all 64 clips (a uniform address: one broadcast read per wave and
//  step), i.e. the weights are read once per tile of 64 clips instead of once per clip.  Layer 0 reads its clip's row from HBM (the feature
//  matrix or the trunk's hand-off); hidden outputs live in LDS as [unit][64 clips] (conflict-free: lane = clip), ping-pong.
// ---------------------------------------------------------------------------------------------------------
constexpr int KWS_DENSEF_WAVES = 4;
constexpr int KWS_DENSEF_UB = 4;

template <bool FIRST>
__device__ __forceinline__ void densef_layer(const KwsDenseLayerF32 &L, const float *__restrict__ xrow, const float *src, float *dst, int lane, int wave)
{
    const int K = L.k;
    for (int o0 = wave * KWS_DENSEF_UB; o0 < L.units; o0 += KWS_DENSEF_WAVES * KWS_DENSEF_UB) {
        const float *wr[KWS_DENSEF_UB];
#pragma unroll
        for (int u = 0; u < KWS_DENSEF_UB; ++u) wr[u] = L.w + (size_t)min(o0 + u, L.units - 1) * K;     // (units past the layer: a copy of the last, not stored)
        float total[KWS_DENSEF_UB];
#pragma unroll
        for (int u = 0; u < KWS_DENSEF_UB; ++u) total[u] = 0.0f;
        int d = 0;
        for (; d + 4 <= K; d += 4) {                      // four steps' operands in flight; every chain stays in order
            float xv[4], wv[KWS_DENSEF_UB][4];
#pragma unroll
            for (int q = 0; q < 4; ++q) xv[q] = FIRST ? xrow[d + q] : src[(d + q) * 64 + lane];
#pragma unroll
            for (int u = 0; u < KWS_DENSEF_UB; ++u)
#pragma unroll
                for (int q = 0; q < 4; ++q) wv[u][q] = wr[u][d + q];
#pragma unroll
            for (int q = 0; q < 4; ++q)
#pragma unroll
                for (int u = 0; u < KWS_DENSEF_UB; ++u) {
                    const float prod = xv[q] * wv[u][q];
                    total[u] += prod;
                }
        }
        for (; d < K; ++d) {
            const float xv = FIRST ? xrow[d] : src[d * 64 + lane];
#pragma unroll
            for (int u = 0; u < KWS_DENSEF_UB; ++u) {
                const float prod = xv * wr[u][d];
                total[u] += prod;
            }
        }
#pragma unroll
        for (int u = 0; u < KWS_DENSEF_UB; ++u)
            if (o0 + u < L.units) dst[(o0 + u) * 64 + lane] = act_clamp(total[u] + L.bias[o0 + u], L.lo, L.hi);
    }
}

__host__ __device__ inline size_t kws_dense_f32_smem_bytes(const KwsDensePlanF32 &D) { return (size_t)(D.buf_floats[0] + D.buf_floats[1]) * 64 * sizeof(float); }

// x: by_clip = 1: the feature matrices [n_clips][K]; 0: the trunk's hand-off [ci - ci0][K].  List entries ci0 .. ci1 - 1 are served.
__global__ __launch_bounds__(KWS_WAVE * KWS_DENSEF_WAVES) void kws_dense_f32_kernel(KwsDensePlanF32 D, const float *__restrict__ x, int by_clip, int ci0,
                                                                                   int ci1, int n_clips, float *__restrict__ scores,
                                                                                   float *__restrict__ tap_logits, const int *__restrict__ sel)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int n_end = min(sel_count(sel, n_clips), ci1);
    float *buf0 = (float *)smem_raw, *buf1 = buf0 + D.buf_floats[0] * 64;
    const int n_labels = D.n_labels;
    for (int cb = ci0 + (int)blockIdx.x * 64; cb < n_end; cb += (int)gridDim.x * 64) {
        // lanes past the batch repeat the last clip (computed, never stored)
        const int ci = min(cb + lane, n_end - 1);
        const bool valid = cb + lane < n_end;
        const int clip = sel_clip(sel, ci);
        const float *xrow = x + (size_t)(by_clip ? clip : ci - ci0) * D.l[0].k;
        densef_layer<true>(D.l[0], xrow, nullptr, buf0, lane, wave);
        __syncthreads();
#pragma unroll
        for (int l = 1; l < KWS_DENSE_MAX; ++l) {
            if (l < D.n_layers) {
                densef_layer<false>(D.l[l], nullptr, (l & 1) ? buf0 : buf1, (l & 1) ? buf1 : buf0, lane, wave);
                __syncthreads();
            }
        }
        float *lg = ((D.n_layers - 1) & 1) ? buf1 : buf0;
        if (wave == 0) {
            // softmax.h:31-63: max, then sum += exp((x - max) * beta) in class order, then exp(...) / sum
            float mx = -FLT_MAX;
            for (int c = 0; c < n_labels; ++c) { const float v = lg[c * 64 + lane]; mx = mx < v ? v : mx; }
            float sum = 0.0f;
            for (int c = 0; c < n_labels; ++c) {
                const float v = lg[c * 64 + lane];
                if (tap_logits && valid) tap_logits[(size_t)clip * n_labels + c] = v;
                const float e = expf((v - mx) * D.beta);
                lg[c * 64 + lane] = e;
                sum += e;
            }
            if (valid)
                for (int c = 0; c < n_labels; ++c) scores[(size_t)clip * n_labels + c] = lg[c * 64 + lane] / sum;
        }
        __syncthreads();
    }
}

size_t kws_nn_f32_smem_bytes(const KwsNnPlanF32 &N, int n_waves)
{
    const NnfLayout L = nnf_layout(N);
    return ((size_t)L.w_floats + L.fc_floats + (size_t)n_waves * (L.a_floats + L.b_floats + L.y_floats + L.vec_floats)) * sizeof(float);
}

// (TB, OB) of a conv block: fewest lane passes x chain work, LDS reads as the tie breaker
void kws_nn_f32_pick_blocking(KwsConvBlockF32 *k)
{
    static const int tbs[] = { 1, 2, 4, 7, 8 }, obs[] = { 1, 2, 4 };
    // a lane that owns exactly one pooling window can max-pool in registers (no staging buffer, fewer LDS bytes per wave);
    // taken when that blocking costs no more than the best free one
    const bool can_fuse = k->pool > 1 && k->pool == k->pool_stride &&
                          (k->pool == 2 || k->pool == 4 || k->pool == 7 || k->pool == 8);
    float best[2] = { 1e30f, 1e30f };
    int btb[2] = { 1, 1 }, bob[2] = { 1, 1 };
    for (int fused = 0; fused < 2; ++fused)
        for (int tb : tbs)
            for (int ob : obs) {
                if (k->depthwise && ob != 1) continue;
                if (fused && (!can_fuse || tb != k->pool)) continue;
                const int n_tb = fused ? k->pool_w : (k->out_w + tb - 1) / tb;
                const int items = n_tb * ((k->out_c + ob - 1) / ob);
                const int passes = (items + 63) / 64;
                const float cost = (float)passes * (2.0f * tb * ob + 1.0f * (tb + 1));
                if (cost < best[fused]) { best[fused] = cost; btb[fused] = tb; bob[fused] = ob; }
            }
    k->fused_pool = (can_fuse && best[1] <= best[0]) ? 1 : 0;
    k->tb = btb[k->fused_pool];
    k->ob = bob[k->fused_pool];
    k->ntb = nnf_ntb_of(*k);
    k->rows = nnf_rows_of(*k);
    // the kernel's item splits: items = time blocks x channel blocks (conv) or x out_c (depthwise, the pooling pass: out_w x out_c at most)
    const long n_ob = k->depthwise ? k->out_c : (k->out_c + k->ob - 1) / k->ob;
    // a reciprocal is used only where x * d < 2^20 (the quotient is then exact) AND x * inv fits nnf_div's 32-bit product (x / d below ~4096:
    // a single channel block with thousands of time blocks would pass the first test and overflow the second -- ADVICE round 5)
    auto recip20 = [](long x_max, long d) -> unsigned {
        const unsigned long inv = (1ul << 20) / (unsigned long)d + 1ul;
        return (x_max * d < (1L << 20) && (unsigned long)x_max * inv < (1ul << 32)) ? (unsigned)inv : 0u;
    };
    k->inv_item20 = recip20((long)k->ntb * n_ob + 64, n_ob);
    k->inv_outc20 = recip20((long)std::max(k->ntb * std::max(k->tb, 1), k->out_w) * k->out_c + 64, k->out_c);
}

long long *kws_dev_f32_prof = nullptr;      // development aid: device buffer of KWS_MAX_BLOCKS + 2 phase counters, or NULL

// waves per workgroup: as many as fit the CU's 160 KB of LDS (they share one copy of the weights), at most 16
int kws_nn_f32_waves(const KwsNnPlanF32 &N)
{
    // a conv block with a channel count that is a multiple of 4 wants the 256-register build (16-byte activation reads),
    // which serves at most 8 waves per workgroup
    bool vec4 = false;
    for (int b = 0; b < N.n_blocks; ++b) vec4 |= !N.blk[b].depthwise && N.blk[b].tb > 1 && (N.blk[b].in_c & 3) == 0;
    for (int w = vec4 ? 8 : 16; w > 4; --w)
        if (kws_nn_f32_smem_bytes(N, w) <= 158 * 1024) return w;
    return 4;
}

// The form of kws_nn_f32_kernel that serves a graph, chosen ONCE per call: the pointer this returns is the one hipFuncSetAttribute opts in to large LDS
// and the one nnf_launch launches.  trunk: the graph has a dense stack behind its conv blocks; sd: some block is strided or dilated;
// at most 8 waves per workgroup take the 256-register build.
static const void *nnf_kernel_for(bool trunk, bool sd, int n_waves)
{
    static const void *const tab[2][2][2] = {
        { { (const void *)kws_nn_f32_kernel<1024, false, false>, (const void *)kws_nn_f32_kernel<512, false, false> },
          { (const void *)kws_nn_f32_kernel<1024, false, true>, (const void *)kws_nn_f32_kernel<512, false, true> } },
        { { (const void *)kws_nn_f32_kernel<1024, true, false>, (const void *)kws_nn_f32_kernel<512, true, false> },
          { (const void *)kws_nn_f32_kernel<1024, true, true>, (const void *)kws_nn_f32_kernel<512, true, true> } } };
    return tab[trunk][sd][n_waves <= 8];
}
// (every form has the one argument list; a form ignores the arguments that are not its own)
static void nnf_launch(const void *fn, int grid, int n_waves, size_t smem, hipStream_t stream, const KwsNnPlanF32 *d_plan, const float *features, int n_clips,
                       float *scores, float *tap_logits, float *handoff, int ci0, int ci1, const int *sel)
{
    void *args[] = { &d_plan, &features, &n_clips, &scores, &tap_logits, &handoff, &ci0, &ci1, &kws_dev_f32_prof, &sel };
    (void)hipLaunchKernel(fn, dim3(grid), dim3(KWS_WAVE * n_waves), args, smem, stream);
}

// A graph with a dense stack: the conv blocks (if any) in the trunk form of kws_nn_f32_kernel, chunk by chunk of the hand-off buffer, each chunk followed
// by kws_dense_f32_kernel over the same list entries.
static int launch_dense_f32(const KwsNnPlanF32 &N, const KwsNnPlanF32 *d_plan, const float *features, int n_clips, float *scores, float *tap_logits,
                            int n_cu, hipStream_t stream, const int *sel)
{
    const KwsDensePlanF32 &D = *N.dense;
    const size_t dsmem = kws_dense_f32_smem_bytes(D);
    if (dsmem > 64 * 1024) {
        hipError_t e = hipFuncSetAttribute((const void *)kws_dense_f32_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)dsmem);
        if (e != hipSuccess) return (int)e;
    }
    auto dense_grid = [&](int n) { const int g = (n + 63) / 64; return g > n_cu * 8 ? n_cu * 8 : g; };
    const KwsNn2dPlanF32 *const trunk2d = N.handoff->trunk2d_f32;     // a 2-D graph: kws_nn2d_f32_trunk_kernel fills the hand-off
    const KwsResPlanF32 *const trunkres = N.handoff->trunkres_f32;   // a residual graph: kws_nnres_f32_trunk_kernel fills the hand-off
    if (N.n_blocks == 0 && !trunk2d && !trunkres) {
        hipLaunchKernelGGL(kws_dense_f32_kernel, dim3(dense_grid(n_clips)), dim3(KWS_WAVE * KWS_DENSEF_WAVES), dsmem, stream, D, features, 1, 0, n_clips, n_clips,
                           scores, tap_logits, sel);
        return (int)hipGetLastError();
    }
    float *ho = (float *)kws_handoff_for(N.handoff, (void *)stream);
    if (!ho) return (int)hipErrorOutOfMemory;
    if (trunk2d || trunkres) {
        if (trunk2d ? !kws_launch_nn2d_f32_trunk : !kws_launch_nnres_f32_trunk) return (int)hipErrorInvalidDeviceFunction;      // (linked without the trunk's unit: kws_nn2d.h, kws_nnres.h)
        const int chunk = (int)(N.handoff->bytes / (sizeof(float) * (size_t)N.fc_in));
        for (int c0 = 0; c0 < n_clips; c0 += chunk) {
            const int c1 = n_clips - c0 > chunk ? c0 + chunk : n_clips;
            int rc = trunk2d ? kws_launch_nn2d_f32_trunk(*trunk2d, features, n_clips, ho, c0, c1, sel, n_cu, stream)
                             : kws_launch_nnres_f32_trunk(*trunkres, features, n_clips, ho, c0, c1, sel, n_cu, stream);
            if (rc) return rc;
            hipLaunchKernelGGL(kws_dense_f32_kernel, dim3(dense_grid(c1 - c0)), dim3(KWS_WAVE * KWS_DENSEF_WAVES), dsmem, stream, D, (const float *)ho, 0, c0, c1, n_clips,
                               scores, tap_logits, sel);
            if ((rc = (int)hipGetLastError())) return rc;
        }
        return 0;
    }
    const int n_waves = kws_nn_f32_waves(N);
    const size_t smem = kws_nn_f32_smem_bytes(N, n_waves);
    const int per_cu = (int)std::max<size_t>(1, (160 * 1024) / smem);
    const void *fn = nnf_kernel_for(true, kws_nnf_strided(N) != 0, n_waves);
    if (smem > 64 * 1024) {
        hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
        if (e != hipSuccess) return (int)e;
    }
    const int chunk = (int)(N.handoff->bytes / (sizeof(float) * (size_t)N.fc_in));            // >= 1024 clips at KWS_HANDOFF_BYTES
    for (int c0 = 0; c0 < n_clips; c0 += chunk) {
        const int c1 = n_clips - c0 > chunk ? c0 + chunk : n_clips, n = c1 - c0;
        int grid = (n + n_waves - 1) / n_waves;
        if (grid > n_cu * per_cu) grid = n_cu * per_cu;
        nnf_launch(fn, grid, n_waves, smem, stream, d_plan, features, n_clips, nullptr, nullptr, ho, c0, c1, sel);
        hipLaunchKernelGGL(kws_dense_f32_kernel, dim3(dense_grid(n)), dim3(KWS_WAVE * KWS_DENSEF_WAVES), dsmem, stream, D, (const float *)ho, 0, c0, c1, n_clips,
                           scores, tap_logits, sel);
        const int rc = (int)hipGetLastError();
        if (rc) return rc;
    }
    return 0;
}

int kws_launch_nn_f32(const KwsNnPlanF32 &N, const KwsNnPlanF32 *d_plan, const float *features, int n_clips, float *scores,
                      float *tap_logits, int n_cu, hipStream_t stream, const int *sel)
{
    (void)hipGetLastError();      // the status returned below is this launch's, not a stale error of an earlier call
    if (n_clips <= 0) return 0;
    if (kws_nnf_dense(N)) return launch_dense_f32(N, d_plan, features, n_clips, scores, tap_logits, n_cu, stream, sel);
    const int n_waves = kws_nn_f32_waves(N), grid_mult = 1;
    const size_t smem = kws_nn_f32_smem_bytes(N, n_waves);
    const int per_cu = (int)std::max<size_t>(1, (160 * 1024) / smem);
    int grid = (n_clips + n_waves - 1) / n_waves;
    if (grid > n_cu * per_cu * grid_mult) grid = n_cu * per_cu * grid_mult;
    const void *fn = nnf_kernel_for(false, kws_nnf_strided(N) != 0, n_waves);
    if (smem > 64 * 1024) {                    // opt in to more than the default 64 KB of dynamic LDS
        hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
        if (e != hipSuccess) return (int)e;
    }
    nnf_launch(fn, grid, n_waves, smem, stream, d_plan, features, n_clips, scores, tap_logits, nullptr, 0, 0, sel);
    return (int)hipGetLastError();
}
