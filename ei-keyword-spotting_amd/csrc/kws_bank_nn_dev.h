// kws_bank_nn_dev.h -- device code shared by the kernels that run int8 members of the two-block matrix-core shape from ONE float feature
// matrix: the bank's (kws_bank_kernels.hip) and the pool's (kws_pool_kernels.hip).  Include it after kws_device.h, kws_nn_int8_dev.h and
// kws_bank.h.  What is here is what a workgroup does once for its member (bank_nn_stage), what a wave does per feature row before
// nn_mfma_clip takes over (bank_quantize_row), and the LDS both need (KWS_BANK_NN_LDS); each kernel keeps its own loop over rows.
#pragma once

// One clip's float feature row src [time][in_c] (F values) -> int8 LDS rows of CP bytes at row (time + pad_left) of act1, quantised with
// quantize_feature (the expression of every other path) -- no int8 tensor goes through HBM.  inv_c: i / in_c == (i * inv_c) >> 20 for
// i < n_features <= 4096.  quads: four channels per load and store where the rows allow it (feature rows and activation rows 16- / 4-byte
// aligned).
template <int CP>
__device__ __forceinline__ void bank_quantize_row(const float *__restrict__ src, int8_t *act1, int F, int in_c, int pad_left, unsigned inv_c, bool quads,
                                                  float in_scale, int in_zp, int lane)
{
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
}

// What a workgroup does once before its waves take clips: the member's head and ADD tables into LDS, the wave's padding rows, its context.
template <int CP>
__device__ __forceinline__ NnHeadTab bank_nn_stage(const KwsNnPlan &N, unsigned char *s_head, int8_t *s_lut1, int8_t *s_lut2, int8_t *act1, int8_t *act2,
                                                   NnMfmaCtx<CP> &ctx, int lane)
{
    const KwsConvBlock &k1 = N.blk[0], &k2 = N.blk[1];
    const NnHeadTab head = nn_head_stage(N, s_head);
    for (int i = threadIdx.x * 4; i < k1.out_c * 256; i += blockDim.x * 4) *(int *)(s_lut1 + i) = *(const int *)(k1.add_lut + i);
    for (int i = threadIdx.x * 4; i < k2.out_c * 256; i += blockDim.x * 4) *(int *)(s_lut2 + i) = *(const int *)(k2.add_lut + i);
    nn_mfma_fill_padding<CP>(N, act1, act2, lane);
    nn_mfma_init<CP>(ctx, N, lane);
    __syncthreads();
    return head;
}

// LDS of one workgroup: the member's ADD tables and head, and per wave the two activation images and the pooled vector
#define KWS_BANK_NN_LDS(CP)                                                                  \
    __shared__ __attribute__((aligned(16))) int8_t s_lut1[32 * 256];                         \
    __shared__ __attribute__((aligned(16))) int8_t s_lut2[16 * 256];                         \
    __shared__ __attribute__((aligned(16))) int8_t s_act1[KWS_NN_WAVES][KWS_A1_ROWS * CP];   \
    __shared__ __attribute__((aligned(16))) int8_t s_act2[KWS_NN_WAVES][KWS_A2_ROWS * 32];   \
    __shared__ int s_vec[KWS_NN_WAVES][64];                                                  \
    __shared__ __attribute__((aligned(16))) unsigned char s_head[KWS_HEAD_BYTES]
