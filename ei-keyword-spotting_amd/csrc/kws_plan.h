// kws_plan.h -- host <-> device execution plans (internal to libkws_mi355x.so).
//
// All tables are built ONCE on the host, in the same precision and order the reference builds them per clip
// ("batch-first, table-once, fused"), uploaded to HBM, and referenced from these structs.
#pragma once
#include <stdlib.h>

// Development switches (environment variables KWS_DEV_*: occupancy experiments, A/B runs, forcing a tier in a test) exist only in a library
// built with -DKWS_DEV_SWITCHES (make dev -> libkws_mi355x_dev.so); the product library does not read the environment and does not
// contain their names.
#ifdef KWS_DEV_SWITCHES
#define KWS_DEV_ENV(name) getenv(name)
#else
#define KWS_DEV_ENV(name) ((const char *)nullptr)
#endif
#include <stdint.h>

struct KwsDspPlan {
    int n_samples;      // EI_CLASSIFIER_RAW_SAMPLE_COUNT (16000)
    int n_frames;       // speechpy numframes (49)                      processing.hpp:260-284
    int frame_stride;   // samples (320)
    int frame_len;      // samples fetched per frame (320); only min(frame_len, fft_len) are used
    int fft_len;        // 256
    int n_bins;         // fft_len/2+1
    int n_filters;      // 32
    int n_cepstral;     // 13
    int win_size;       // 101
    int pad;            // (win_size-1)/2
    int pre_shift;      // 1
    float pre_cof;      // 0.98
    float inv_fft;      // 1/fft_len (power of two => exact)
    float dct_s0, dct_s1;   // sqrtf(1/(4N)), sqrtf(1/(2N))                numpy.hpp:392-397
    int max_nz;         // longest mel filter (non-zero taps)
    int filt_nnz;       // non-zero weights of the whole filterbank (length of filt_bin / filt_w)
    // device tables
    const float2 *tw;        // [fft_len/2]  kiss_fft twiddles              kiss_fft.cpp:351-357
    const float2 *stw;       // [fft_len/4]  kiss_fftr super twiddles       kiss_fftr.cpp:52-58
    const int *filt_start;   // [n_filters+1] CSR over the transposed filterbank, ascending bin
    const int *filt_bin;
    const float *filt_w;
    const float2 *dct_tw;    // [n_filters/2]
    const float2 *dct_stw;   // [n_filters/4]
    const float *dct_cos;    // [n_filters/2+1] cosf((float)(i*pi/(2N)))    fast-dct-fft.cpp:71-74
    const float *dct_sin;
    const int *pad_map;      // [n_frames+2*pad] numpy::pad_1d_symmetric row map   numpy.hpp:479-541
    // configurations outside the tuned kernel's instantiations run on the general kernels (kws_generic.hip): kf_factor's factor
    // lists (kiss_fft.cpp:303-324: p, m pairs) of the frame transform (fft_len / 2 points) and of the DCT's (n_filters / 2 points)
    int generic;
    // generic = 1, but the SPECTRAL stage alone fits the tuned kernel's instantiations (fft 256, 32 / 40 filters, aligned frames, short mel filters) -- what
    // makes the plan general is its frame count or its cmvnw window: int16 windows then take kws_mfcc8_kernel over chunks of at most kws_mfcc_max_frames
    // frames (frames are independent but for pre-emphasis' predecessor sample, below) and only cmvnw runs on the general kernel (round 6; kws_api.cpp)
    int spectral_tuned;
    // kws_mfcc8_kernel, the window's first sample: its predecessor is x[wrap_index] of the window -- n_samples - 1, the reference's wrap
    // (processing.hpp:68, 104-106) -- unless the launch names another (a chunk that starts inside the window: -1, the sample before it)
    int wrap_index;
    int fft_levels, dct_levels;
    int fft_fac[24], dct_fac[24];
    // per launch, continuous mode: the rolling feature buffer of a stream is a ring over its first ring_rows rows (the rows behind
    // them are the reference's never-written tail).  Producers (WITH_CMVN = false, MFE rows): output row r goes to physical row
    // (ring_row0 + r) % ring_rows; consumers (kws_cmvn_nn_kernel, kws_unring_kernel): logical row i < ring_rows is physical row
    // (i + ring_head) % ring_rows.  ring_rows = 0: plain rows.
    int ring_rows, ring_row0, ring_head;
    // per launch, WITH_CMVN = false only: when set the kernel stops after speechpy::feature::mfe (feature.hpp:193-318)
    // and writes the mel energies [window][frame][filter] and frame energies [window][frame] (both after zero handling)
    float *mfe_mel, *mfe_energy;
};

// One "conv block" of the Edge Impulse 1-D CNN family:
//   RESHAPE -> CONV_2D(1xK) | DEPTHWISE_CONV_2D(1xK) -> RESHAPE -> [ADD(bias, ReLU)] -> RESHAPE -> [MAX_POOL_2D(P)] -> RESHAPE
#define KWS_MAX_BLOCKS 8
struct KwsConvBlock {
    int in_w, in_c, in_cpad;   // time steps, channels, channels padded to a multiple of 16
    int out_c;
    int taps, pad_left;        // filter width, SAME padding on the left
    int out_w;                 // conv output width
    int pool, pool_stride, pool_w;   // pool window, stride, pooled width
    int in_zp;                 // input zero point (= padding value so that (x + offset) == 0)
    int out_zp, act_min, act_max;    // conv output zero point and clamp
    int depthwise, depth_mult; // DEPTHWISE_CONV_2D: output channel oc reads input channel oc / depth_mult
    int has_lut;               // an ADD follows the convolution (add_lut is not the identity)
    int mfma;                  // generic kernel: this block's convolution runs on the matrix cores (CONV_2D, no pooling,
                               // in_cpad 16 / 32 / 64, out_c <= 32, out_w <= 64)
    int w_bytes;               // bytes of w
    short stride, dilation;    // along time: output t, tap j reads padded-image row t * stride + j * dilation.  A block with either above 1 never sets
                               // mfma, and its graph runs on the strided forms of the generic kernel (kws_nn_sd_kernel, kws_nn_sd_trunk_kernel).  Two 16-bit
                               // fields (the plan bounds both below 4096) in the four bytes that padded w_bytes up to the pointers: the struct the stride-1
                               // kernels take by value keeps its size and every offset, and with them their code objects (profiles/strided_codeobj.md)
    const int8_t *w;           // conv: [out_c][taps][in_cpad], zero padded; depthwise: [out_c][taps padded to 4]
    const int32_t *bias_eff;   // [out_c] bias + input_offset * sum(w)
    const int32_t *mult;       // [out_c] per-channel quantized multiplier
    const int32_t *shift;      // [out_c]
    const int8_t *add_lut;     // [out_c][256] ADD(bias tensor)+ReLU folded: out = lut[c][x+128]
};

// FULLY_CONNECTED limits: input vector length, and weights per model (their LDS copy: bytes for int8, floats * 4 for float32)
#define KWS_FC_IN_MAX 1024
#define KWS_FC_W_MAX 32768

// Dense stacks: graphs that end in 2 .. 4 FULLY_CONNECTED layers, or whose FULLY_CONNECTED layers (1 .. 4) follow no conv block.  kws_dense_i8_kernel / kws_dense_f32_kernel run the whole chain for a tile of clips; conv blocks in front of it run in the trunk form of
// the generic kernels, which stops at the last block's output ([clips][inputs] in HBM, KwsHandoff).
#define KWS_DENSE_MAX 4
#define KWS_DENSE_UNITS_MAX 256            // a hidden layer's units (the last layer: labels <= 48)
#define KWS_DENSE_IN_MAX 4096              // inputs of the first layer
#define KWS_DENSE_W_MAX (1 << 20)          // bytes of weights per layer
#define KWS_DENSE_LDS_W (64 * 1024)        // int8: fragment bytes kept in LDS (layers that do not fit are read from L2)
struct KwsDenseLayer {
    int k, kpad;               // inputs, padded to the matrix instruction's 64
    int units, upad;           // outputs, padded to a 16-column tile
    int w_off;                 // -weight zero point: w_off * sum(x) is added per clip
    int out_zp, mult, shift, act_min, act_max;
    int lds_off;               // byte offset of the fragments in the workgroup's LDS block, or -1: read from L2
    const int8_t *wfrag;       // [upad / 16][kpad / 64][64 lanes][16]: lane l holds w[16 t + (l & 15)][64 s + 16 (l >> 4) .. + 15], zero padded
    const int32_t *bias_eff;   // [upad] bias + in_off * sum(w) + k * in_off * w_off
};
struct KwsDensePlan {
    int n_layers, n_labels;
    int lds_w_bytes;           // fragments staged in LDS
    int act_stride;            // bytes per clip row of the per-wave activation buffers (a multiple of 16 that is no multiple of 64)
    int tap_off;               // where the hidden layers' outputs start in a clip's tap_pooled row (= the conv blocks' pooled bytes)
    KwsDenseLayer l[KWS_DENSE_MAX];
    const int32_t *sm_exp;     // as KwsNnPlan
    const uint8_t *sm_valid;
    float out_scale;
    int out_zp;
};
struct KwsDenseLayerF32 {
    int k, units;
    float lo, hi;              // fused activation range
    const float *w;            // [units][k]
    const float *bias;         // [units] (zeros where the node has none: the reference adds 0.0f)
};
struct KwsDensePlanF32 {
    int n_layers, n_labels;
    float beta;
    int buf_floats[2];         // per clip: the widest output of the even / odd layers
    KwsDenseLayerF32 l[KWS_DENSE_MAX];
};
struct KwsHandoff;             // kws_plan.cpp: the trunk's output buffers, one per stream

struct KwsNnPlan {
    int n_blocks;
    KwsConvBlock blk[KWS_MAX_BLOCKS];
    int n_features;            // 637
    int fc_in, fc_out;
    int fc_in_off, fc_w_off, fc_out_zp, fc_mult, fc_shift, fc_act_min, fc_act_max;
    // fc_out == 0: the graph ends in a dense stack, not in the head above; the head's two pointers then name the stack's plan and the trunk's hand-off
    // buffers (host pointers, owned by the handle) -- kws_nn_dense().  A union, so that the struct the existing kernels take by value keeps its layout.
    union { const int8_t *fc_w; const KwsDensePlan *dense; };          // fc_w: [fc_out][fc_in]
    union { const int32_t *fc_bias; KwsHandoff *handoff; };            // fc_bias: [fc_out]
    // softmax (int8 -> int8): exp LUT indexed by (max - x) in [0,255]; 0 where diff < diff_min
    const int32_t *sm_exp;     // [256] exp_on_negative_values(rescaled diff), Q0.31
    const uint8_t *sm_valid;   // [256] diff >= diff_min
    float in_scale;            // input tensor quantisation (ei_run_classifier.h:436-444)
    int in_zp;
    float out_scale;           // output dequantisation
    int out_zp;
    int n_labels;
};
static inline const KwsDensePlan *kws_nn_dense(const KwsNnPlan &N) { return N.fc_out == 0 ? N.dense : nullptr; }
// some block of the graph is strided or dilated: the graph runs on the strided forms of the generic kernels, never on a matrix-core or fast-mode kernel
static inline int kws_nn_strided(const KwsNnPlan &N)
{
    for (int b = 0; b < N.n_blocks; ++b)
        if (N.blk[b].stride != 1 || N.blk[b].dilation != 1) return 1;
    return 0;
}

// ---- float32 models (the reference's float TFLite-Micro kernels: reference/conv.h:28-99, add.h:179-215,
//      pooling.h:189-237, fully_connected.h:26-60, softmax.h:31-63) -------------------------------------------
struct KwsConvBlockF32 {
    int in_w, in_c, out_c, taps, pad_left, out_w;
    int pool, pool_stride, pool_w;
    int has_add;
    int depthwise, depth_mult;     // DEPTHWISE_CONV_2D (filter [1][1][taps][out_c]); else CONV_2D (filter [out_c][1][taps][in_c])
    int tb, ob;                    // register blocking of the conv: time steps x output channels per lane
    int fused_pool;                // tb == pool == pool_stride: the lane max-pools its own window, no staging of the conv output
    unsigned inv_item20, inv_outc20;   // 2^20 / d + 1 for the kernel's item splits (d = channel blocks per time block, or out_c), 0 where items x d >= 2^20
    int ntb, rows;                 // set with the blocking (kws_nn_f32_pick_blocking): time blocks per channel block, rows of the zero-padded input image
                                   // -- derived values the kernel would otherwise divide for on every clip (a 32-bit division is ~35 vector instructions)
    float conv_min, conv_max;      // fused activation range of the convolution
    float add_min, add_max;        // fused activation range of the ADD (ReLU: [0, max])
    float pool_min, pool_max;
    short stride, dilation;        // along time, as KwsConvBlock's (kws_nn_f32_sd_kernel, kws_nn_f32_sd_trunk_kernel): in the four bytes that padded pool_max up to
                                   // the pointers, so that the plan the stride-1 kernels read keeps every offset
    const float *w;                // conv: [out_c][taps][in_c]; depthwise: [taps][out_c]
    const float *bias;             // [out_c]
    const float *addc;             // [out_c] constant operand of the ADD
};

struct KwsNnPlanF32 {
    int n_blocks;
    KwsConvBlockF32 blk[KWS_MAX_BLOCKS];
    int n_features, fc_in, fc_out, n_labels;
    float fc_min, fc_max, beta;
    union { const float *fc_w; const KwsDensePlanF32 *dense; };       // [fc_out][fc_in]; fc_out == 0: as KwsNnPlan (kws_nnf_dense())
    union { const float *fc_bias; KwsHandoff *handoff; };             // [fc_out]
};
static inline const KwsDensePlanF32 *kws_nnf_dense(const KwsNnPlanF32 &N) { return N.fc_out == 0 ? N.dense : nullptr; }
static inline int kws_nnf_strided(const KwsNnPlanF32 &N)
{
    for (int b = 0; b < N.n_blocks; ++b)
        if (N.blk[b].stride != 1 || N.blk[b].dilation != 1) return 1;
    return 0;
}
// ---- 2-D convolutional graphs: CONV_2D (KH x KW, both spatial axes live) [-> MAX_POOL_2D] blocks in front of a dense stack.  Plans of
//      their own -- the structs above are taken by value by the 1-D kernels and keep their layout -- read by kws_nn2d_trunk_kernel (kws_nn2d_int8.hip) /
//      kws_nn2d_f32_trunk_kernel (kws_nn2d_f32.hip) alone.  The graph's KwsNnPlan / KwsNnPlanF32 has n_blocks = 0 and its dense stack; the trunk is
//      reached through the hand-off (KwsHandoff::trunk2d / trunk2d_f32): the trunk is what fills those buffers.
#define KWS_NN2D_K_MAX 7                   // filter and pool window, per axis
#define KWS_NN2D_STRIDE_MAX 4              // convolution stride, per axis (pool strides: up to KWS_NN2D_K_MAX)
#define KWS_NN2D_DIM_MAX 1024              // image height / width (bounds every product of the geometry far inside an int)
struct KwsConv2dGeom {
    int in_h, in_w, in_c, out_c;
    int kh, kw, sh, sw, pad_t, pad_l;      // filter, stride, SAME padding above / left of the image (kernels/padding.h)
    int out_h, out_w;                      // conv output
    int ph, pw, psh, psw, ppt, ppl;        // pool window, stride, padding above / left (no pooling node: 1, 1, 1, 1, 0, 0)
    int pool_h, pool_w;                    // pooled output (= out_h, out_w without a pooling node)
    int has_pool;                          // a MAX_POOL_2D follows (float: a window of one value still goes through std::max and the pool's clamp)
    int img_rows, img_cols;                // the padded input image in LDS: rows x columns (pixels) -- what the furthest tap of the furthest output reads
    int img_pitch;                         // elements (bytes / floats) per image row: img_cols * in_c rounded up to an ODD number of dwords, so that the rows a
                                           // wave's lanes read at once start on different LDS banks
    int krow, krow4;                       // operands of one filter row: kw * in_c, and rounded up to a multiple of 4 (int8: dot4 words; zero weights)
};
struct KwsConv2dBlock {
    KwsConv2dGeom g;
    int in_zp, out_zp, act_min, act_max;
    int w_bytes;
    const int8_t *w;                       // [out_c][kh][krow4], zero padded
    const int32_t *bias_eff;               // [out_c] bias + input_offset * sum(w)
    const int32_t *mult, *shift;           // [out_c]
};
struct KwsNn2dPlan {
    int n_blocks, n_features, out_n;       // out_n: the last block's pooled output, flattened NHWC (= the dense stack's inputs)
    int tap_bytes;                         // of every block's pooled output, one after another (the conv blocks' share of tap_pooled)
    KwsConv2dBlock blk[KWS_MAX_BLOCKS];
};
struct KwsConv2dBlockF32 {
    KwsConv2dGeom g;
    float conv_min, conv_max, pool_min, pool_max;
    const float *w;                        // [out_c][kh][krow] (the filter tensor as it is)
    const float *bias;                     // [out_c] (zeros where the node has none: the reference adds 0.0f)
};
struct KwsNn2dPlanF32 {
    int n_blocks, n_features, out_n;
    KwsConv2dBlockF32 blk[KWS_MAX_BLOCKS];
};
// bytes of image b's LDS buffer: the padded image plus 16 bytes the last filter row's zero-weight tail may read (int8), rounded to 16
__host__ __device__ static inline int kws_nn2d_img_bytes(const KwsConv2dGeom &g, int elem) { return (g.img_rows * g.img_pitch * elem + 16 + 15) & ~15; }

// ---- residual graphs and depthwise-separable 2-D graphs: a list of steps -- CONV_2D, DEPTHWISE_CONV_2D or ADD(tensor, tensor),
//      each [-> MAX_POOL_2D] -- over H x W x C images (H >= 1) in front of a dense stack.  Plans of their own again, read by kws_nnres_trunk_kernel (kws_nnres_int8.hip) / kws_nnres_f32_trunk_kernel
//      (kws_nnres_f32.hip) alone and reached through the hand-off (KwsHandoff::trunkres / trunkres_f32).
//      Every tensor lives ONCE in LDS, in one of KWS_RES_SLOTS per-wave buffers the plan's liveness analysis assigns, behind a margin that is the largest
//      top / left padding any of its consumers needs; a consumer with less padding starts reading further in (a_off / b_off).
#define KWS_RES_SLOTS 4                    // tensors live at once, the one being written included
#define KWS_RES_STEPS_MAX 16
#define KWS_RES_K_MAX 16                   // filter side (the 1-D family's tap bound); pool windows keep KWS_NN2D_K_MAX
#define KWS_RES_CONV 0
#define KWS_RES_ADD 1
#define KWS_RES_DW 2
struct KwsResGeom {
    int kind;                              // KWS_RES_CONV / KWS_RES_ADD / KWS_RES_DW
    int in_c, out_c, kh, kw, sh, sw;       // ADD: in_c = out_c, 1 x 1, stride 1
    int dm;                                // depthwise: the depth multiplier, out_c = in_c * dm and output channel oc reads input channel oc / dm (else 1)
    int out_h, out_w;                      // the step's own output (before the pool)
    int ph, pw, psh, psw, ppt, ppl;        // pool window, stride, padding above / left (no pooling node: 1, 1, 1, 1, 0, 0)
    int pool_h, pool_w, has_pool;
    int krow, krow4;                       // conv: operands of one filter row, kw * in_c, and rounded up to a multiple of 4; depthwise: kw (per channel)
    // sources: where the tensor's slot starts in the wave's LDS region (elements; a multiple of 16 bytes), element offset of the first element the step's
    // output (0, 0) reads (the tensor's margin minus this step's own padding), elements per image row.  ADD: a and b (they may be the same tensor); conv: a
    int a_base, a_off, a_pitch, b_base, b_off, b_pitch;
    // destination: slot start (-1: the hand-off row, flattened NHWC), element offset of pixel (0, 0) behind the tensor's margin, elements per row, and the
    // bytes of the image the step first fills with the tensor's padding value (a multiple of 16)
    int d_base, d_off, d_pitch, d_bytes;
};
struct KwsResStep {
    KwsResGeom g;
    int d_zp;                              // the output tensor's zero point: its image's padding value
    int out_zp, act_min, act_max;
    int add_mult, add_shift;               // ADD: the output multiplier (< 1: add_shift <= 0)
    int w_bytes;
    const int8_t *w;                       // conv: [out_c][kh][krow4], zero padded; depthwise: [kh][kw][out_c], the tensor's own order (w_bytes rounded up to 4)
    const int32_t *rq;                     // conv / depthwise: [out_c] x (bias_eff, multiplier, shift, 0); ADD: two 256-entry tables, q1 of operand a and q2 of operand b
                                           // by value + 128 (integer_ops/add.h: the operand shifted left by 20, through its own multiplier)
};
struct KwsResPlan {
    int n_steps, n_features, out_n;        // out_n: the last step's (pooled) output, flattened NHWC (= the dense stack's inputs)
    int tap_bytes;                         // of every step's (pooled) output, one after another
    int n_adds, n_dw;
    int in_base, in_off, in_pitch, in_bytes, in_zp, in_h, in_row;     // the reshaped input tensor's image: in_h rows of in_row values
    int wave_bytes;                        // LDS per wave: the KWS_RES_SLOTS slots, each a multiple of 16 bytes
    KwsResStep st[KWS_RES_STEPS_MAX];
};
struct KwsResStepF32 {
    KwsResGeom g;
    float act_min, act_max, pool_min, pool_max;     // the convolution's / the ADD's clamp, the pool's
    int w_lds;                             // conv: the filter is staged in LDS (else the lanes read it from HBM through the caches: a float twin's filters can
                                           // exceed the LDS -- the plan spills the largest ones)
    const float *w;                        // [out_c][kh][krow]; depthwise: [kh][kw][out_c] (either way the filter tensor as it is, out_c * kh * krow values)
    const float *bias;                     // [out_c]
};
struct KwsResPlanF32 {
    int n_steps, n_features, out_n, n_adds, n_dw;
    int in_base, in_off, in_pitch, in_bytes, in_h, in_row;
    int wave_bytes;
    KwsResStepF32 st[KWS_RES_STEPS_MAX];
};

// the trunk's output [clips][inputs] for one chunk of clips, per stream (launches on different streams may overlap); allocated on first use, freed with
// the handle
#define KWS_HANDOFF_SETS 8
#define KWS_HANDOFF_BYTES (16u << 20)
struct KwsHandoff {
    struct { void *stream; void *buf; int used; } set[KWS_HANDOFF_SETS];
    int next;
    size_t bytes;              // of every buffer: KWS_HANDOFF_BYTES (the development build reads KWS_DEV_HANDOFF_BYTES at kws_create: tests that walk several chunks)
    // a 2-D graph: the trunk that fills the buffers (host plans owned by the handle), else NULL
    const KwsNn2dPlan *trunk2d;
    const KwsNn2dPlanF32 *trunk2d_f32;
    // a residual graph, likewise
    const KwsResPlan *trunkres;
    const KwsResPlanF32 *trunkres_f32;
};
void *kws_handoff_for(KwsHandoff *H, void *stream);      // kws_plan.cpp; NULL when the allocation fails
