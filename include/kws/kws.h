/*
 * kws.h -- batch extension of the drop-in boundary (last row): the same hot
 * path as run_classifier() (include/kws/ei_compat.h), for B clips resident in HBM, plus model
 * loading (the reference compiles its model in; here it is a .kwsm blob made by tools/eon_import.py
 * from the reference's generated MODEL/tflite-model/trained_model_compiled.cpp:70-328 and
 * MODEL/model-parameters/model_metadata.h:38-132).
 *
 * Streams and concurrency: a handle owns one set of scratch buffers (the int8 input tensor / the cepstra of the combined entry
 * points, the fast mode's clip list).  Calls on ONE handle are ordered by the library: a call enqueued on a different stream than
 * the handle's previous call first makes its stream wait (hipStreamWaitEvent) for that previous call's work, so two streams on
 * one handle are safe but do not overlap; for overlap use one handle per stream.  Growing the scratch (a larger batch than any
 * before) synchronises the device.
 *
 * Plain C ABI: pointers and sizes only.  `*_device` entry points take DEVICE pointers and a
 * hipStream_t passed as void* (NULL = default stream) and are asynchronous; the others take host
 * pointers and synchronise.  All return EI_IMPULSE_ERROR values (0 = EI_IMPULSE_OK).
 */
#ifndef KWS_H
#define KWS_H

#include <stddef.h>
#include <stdint.h>

#include "ei_compat.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct kws_handle kws_handle;

/* Build the execution plan for a model blob on HIP device `device` (tables are computed on the host
 * exactly as the reference computes them per clip -- filterbank feature.hpp:54-171, twiddles
 * kiss_fft.cpp:351-357, requantisation multipliers kernel_util_lite.cc:47-120 ... -- and uploaded once). */
EI_IMPULSE_ERROR kws_create(const void *model_blob, size_t nbytes, int device, kws_handle **out);
EI_IMPULSE_ERROR kws_create_from_file(const char *path, int device, kws_handle **out);
void kws_destroy(kws_handle *h);
const char *kws_last_error(void);          /* thread-local detail string for the last failing call */

int kws_label_count(const kws_handle *h);                /* EI_CLASSIFIER_LABEL_COUNT */
const char *kws_label(const kws_handle *h, int i);       /* ei_classifier_inferencing_categories[i] */
int kws_feature_count(const kws_handle *h);              /* EI_CLASSIFIER_NN_INPUT_FRAME_SIZE */
int kws_clip_samples(const kws_handle *h);               /* EI_CLASSIFIER_RAW_SAMPLE_COUNT */
int kws_frame_count(const kws_handle *h);                /* MFCC rows (49) */
int kws_filter_count(const kws_handle *h);               /* mel filters of the DSP block (32) */
int kws_pooled_tap_bytes(const kws_handle *h);           /* bytes/clip of the pooled-activation tap (hidden dense layers' outputs included) */
int kws_dense_layer_count(const kws_handle *h);          /* FULLY_CONNECTED layers of the graph: 1 for the conv family with its single head, 1 .. 4 for a dense
                                                            stack ([RESHAPE]* . 0 .. 8 conv blocks . 1 .. 4 FULLY_CONNECTED . SOFTMAX; hidden layers of 1 .. 256
                                                            units with any fused activation, with or without bias; at most 4096 inputs and 1 MiB of weights per
                                                            layer; the last layer's outputs are the labels, at most 48; behind conv blocks a stack has at
                                                            least two layers -- a single FULLY_CONNECTED there keeps the conv kernels' head limits).  Such graphs run on kws_dense_i8_kernel /
                                                            kws_dense_f32_kernel; a float32 one has no KWS_MODE_FAST (kws_set_mode: KWS_ERROR_UNSUPPORTED_MODEL).
                                                            Conv blocks in front of a stack hand their output over through a 16 MiB device buffer PER STREAM
                                                            (allocated at a stream's first such call, kept until kws_destroy, at most 8: 128 MiB per handle); a
                                                            larger batch is walked in chunks of that size.  Limits that follow: concurrent calls on one handle
                                                            must use different streams (two threads on ONE stream would share its buffer), and a handle serves
                                                            at most 8 streams without waiting -- a ninth takes over the oldest buffer after a device
                                                            synchronise, which is only safe when no other thread is inside a call on that handle.  Graphs
                                                            without a dense stack, and dense-only graphs, use no such buffer */
/* Conv blocks (every family above): CONV_2D 1xK / 1x1 and DEPTHWISE_CONV_2D over time, each with stride_w >= 1 and dilation_width_factor >= 1 (1 <= stride <=
 * input rows, (taps - 1) * dilation < 4096), int8 and float32; output rows and padding follow kernels/padding.h with the real stride and dilation.  Refused with
 * KWS_ERROR_UNSUPPORTED_MODEL (kws_last_error names the node and the reason): stride_h / dilation_height_factor other than 1; SAME-padded DEPTHWISE_CONV_2D with
 * dilation > 1 (the reference computes that padding with dilation 1, depthwise_conv.cc:489-492, so its result is shifted); an output tensor of another width; a
 * padded input image past the kernels' LDS budget.  A graph with a strided or dilated block runs in KWS_MODE_EXACT only: kws_set_mode(h, KWS_MODE_FAST) returns
 * KWS_ERROR_UNSUPPORTED_MODEL and the handle goes on serving KWS_MODE_EXACT. */
/* 2-D convolutional graphs (Edge Impulse's "2D Convolutional" classifier): the tensor flowing into the first convolution is [1][H][W][C] with H > 1
 * and W > 1 (H: frames, W: cepstral / mel columns, Keras' Reshape((frames, columns, 1))).  1 .. 8 blocks, each CONV_2D (filter KH x KW with 1 <= KH, KW <= 7,
 * stride 1 .. 4 per axis, dilation 1, SAME or VALID, constant bias or none, fused activation 0 .. 3, at most 64 channels in and out, int8 per-channel or per-tensor
 * weights, or float32) optionally followed by MAX_POOL_2D (window and stride 1 .. 7 per axis, SAME or VALID); then a flatten, 1 .. 4 FULLY_CONNECTED within the
 * dense-stack limits above (at most 4096 inputs: a graph whose last block leaves more than that is refused; the stock two-block graph leaves 13 x 4 x 16 = 832 on 49 x 13 features and 13 x 10 x 16 = 2080 on 49 x 40) and SOFTMAX.  Such a graph ALWAYS ends
 * in the dense stack's kernels, a single FULLY_CONNECTED included, so the hand-off buffers and their stream rules above apply.  Refused with
 * KWS_ERROR_UNSUPPORTED_MODEL (kws_last_error names the node and the reason): DEPTHWISE_CONV_2D or a per-channel ADD inside such a graph, dilation other than 1, a
 * filter, stride or pool outside the bounds, an output tensor whose dims disagree with kernels/padding.h, an image that does not fit the kernels' LDS budget at four
 * waves per workgroup, non-finite float weights, an int8 MAX_POOL_2D with a fused activation, and left-shifting requantisation past the bound of the 1-D blocks.
 * KWS_MODE_EXACT only: kws_set_mode(h, KWS_MODE_FAST) returns KWS_ERROR_UNSUPPORTED_MODEL and the handle goes on serving KWS_MODE_EXACT.  No matrix-core
 * kernel serves the blocks: the trunk runs on v_dot4 (int8) / in-order float chains.  tap_pooled of kws_nn_batch_device holds every block's (pooled) output in NHWC
 * order, one after another, then the hidden dense outputs; kws_pooled_tap_bytes says how many. */
int kws_conv2d_block_count(const kws_handle *h);         /* CONV_2D blocks of a 2-D graph; 0 for every other graph */
/* Residual graphs: a graph in which at least one ADD sums two ACTIVATION tensors -- the identity and (strided) 1 x 1 projection shortcuts of
 * TC-ResNet-style spotters and ResNet-ish Keras models, on [1][1][W][C] and on [1][H][W][C] images alike.  Between the input RESHAPE and the flatten the graph is
 * a list of at most 16 steps in node order: CONV_2D (filter sides 1 .. 16, stride 1 .. 4 per axis, dilation 1, SAME / VALID, constant bias or none, fused activation
 * 0 .. 3, at most 64 channels) or ADD(a, b) (identical 4-D dims, any scales and zero points, fused activation 0 .. 3; a and b any earlier tensors, the same one
 * twice included), each optionally followed by a MAX_POOL_2D that is the only reader of its input.  RESHAPEs that keep the quantisation are renamings.  At most 4
 * tensors are live at once.  A flatten, 1 .. 4 FULLY_CONNECTED layers and SOFTMAX follow.  Served bit-exactly (float32: logits bit for bit, scores within 1e-6) by
 * kws_nnres_trunk_kernel / kws_nnres_f32_trunk_kernel in front of the dense kernels, through every entry point.  Refused with KWS_ERROR_UNSUPPORTED_MODEL
 * (kws_last_error names the node and the reason): a broadcasting ADD, a constant ADD operand in such a graph, dilation other than 1, more
 * than 16 steps or 4 live tensors, a pool that shares its input with another reader, an int8 pool with a fused activation, output dims that disagree with
 * kernels/padding.h, non-finite float weights, left-shifting conv requantisation past the 1-D blocks' bound, an int8 ADD whose output multiplier
 * 2 max(s1, s2) / (2^20 s_out) is not below 1, and a graph that does not fit the kernels' LDS budget at two waves per workgroup (four before DESIGN 4.18).  KWS_MODE_EXACT only, as a 2-D
 * graph.  tap_pooled of kws_nn_batch_device holds every step's (pooled) output in step order, then the hidden dense outputs. */
int kws_residual_add_count(const kws_handle *h);         /* tensor + tensor ADDs of a residual graph; 0 for every other graph (kws_conv2d_block_count stays 0 for a residual graph) */
/* Depthwise-separable 2-D graphs and depthwise steps next to a skip connection: the step list above takes a third kind, DEPTHWISE_CONV_2D
 * (filter [1][kh][kw][channels x depth_multiplier], multiplier >= 1, at most 64 output channels, sides 1 .. 16, stride 1 .. 4 per axis, dilation 1, SAME / VALID,
 * constant bias or none, per-channel scales along dimension 3 or one scale), and the same kernels serve a graph when it has a tensor + tensor ADD (as before) OR
 * it is a 2-D graph ([1][H][W][C] input image, H > 1 and W > 1) that holds a DEPTHWISE_CONV_2D -- Hello-Edge DS-CNN, MobileNet-style trunks, MobileNetV2 inverted
 * residuals, MatchboxNet-style separable blocks with a shortcut.  int8 depthwise steps clamp to the int8 range whatever their fused activation says, as the
 * reference's kernel does; float32 ones honour it.  A 1-D graph with depthwise blocks and no tensor + tensor ADD keeps the block kernels (and the fast mode).
 * Refused (the message names the node as "conv N:" and says DEPTHWISE_CONV_2D): a filter of other dims, a multiplier < 1 or one that disagrees with the tensors,
 * more than 64 output channels, dilation, left-shifting requantisation past the 1-D blocks' bound, non-finite float weights.  KWS_MODE_EXACT only. */
int kws_depthwise_step_count(const kws_handle *h);       /* DEPTHWISE_CONV_2D steps of a graph the step trunks serve; 0 for every other graph (a 1-D depthwise chain on the
                                                            block kernels included).  kws_residual_add_count is 0 for a 2-D depthwise graph without ADDs */
const char *kws_nn_kernel_name(const kws_handle *h);    /* which network kernel serves this model (diagnostics); "kws_nn_sd_kernel" / "kws_nn_f32_sd_kernel" (in front of a
                                                            dense stack: "kws_nn_sd_trunk_kernel + kws_dense_i8_kernel", float32 likewise) for a graph with a strided or dilated block;
                                                            "kws_nn2d_trunk_kernel + kws_dense_i8_kernel" / "kws_nn2d_f32_trunk_kernel + kws_dense_f32_kernel" for a 2-D graph.
                                                            The strings are LABELS of the kernels' forms, stable across releases, not device symbols: the generic kernels are
                                                            templates (kws_nn_kernel<MAXW, TRUNK, SD>, kws_nn_f32_kernel<MAXT, TRUNK, SD>) and a profiler shows their instantiations */
const char *kws_mfcc_kernel_name(const kws_handle *h);  /* the spectral kernel of int16 batches, MFCC and MFE blocks alike: "kws_mfcc8_kernel" / "kws_mfcc_kernel" (tuned shapes), "kws_mfcc8_kernel (chunked)" (general plans whose spectral stage fits the tuned kernel: chunks of at most 49 frames), "kws_spectral_lds_kernel" (general shapes), "kws_spectral_generic_kernel" (those whose arrays exceed the LDS) */
int kws_model_is_float(const kws_handle *h);             /* 1: float32 graph (EI_CLASSIFIER_TFLITE_INPUT_QUANTIZED == 0) */

/* ---- arithmetic mode of the device-resident batch hot path (kws_run_classifier_batch_device, kws_extract_mfcc_batch_device,
 * kws_cmvn_inference_batch_device, kws_streams_step_device).  The host-buffer entry point kws_run_classifier_batch always runs the exact kernels: it is bound by
 * PCIe, the mode would buy nothing there.
 * KWS_MODE_EXACT (default): every floating-point operation replays the reference's order: MFCC features bit-identical, int8 graphs
 *   bit-identical end to end, float32 scores within 1e-6.
 * KWS_MODE_FAST: the tolerance BASELINE.json grants (1e-4 on float32 scores) is spent where the reference's operation order is
 *   expensive: fp32 power spectrum, DCT on the matrix cores, O(1) running-sum cmvnw, and -- float32 graphs of CONV_2D blocks --
 *   the network on v_mfma_f32_16x16x4_f32 in the same launch (the feature matrix never leaves the chip).  The FFT keeps
 *   KissFFT's order.  Clips whose cmvnw is ill-conditioned (near-constant column) are detected and re-run by the exact
 *   kernels inside the same call, so their results are the exact mode's.  int8 graphs: fast MFCC + the exact int8 network;
 *   an int8 input value may then differ by one step where a feature sits on a rounding boundary.
 * kws_streams_step_device follows the mode too (the slice's MFCC stays exact; the whole-window cmvnw + network take the fast
 * kernel).  The SDK entry points (run_classifier ...) and the other stage entry points always run the exact kernels.
 * Models whose DSP block is MFE (extract_mfe_features of the newer SDK copy): KWS_MODE_FAST runs the block's front end -- FFT in
 *   KissFFT's order, fp32 power, fused mel products -- in the fast kernel and keeps the block's normalisation (it divides by the
 *   matrix's range, not by a deviation: nothing is ill-conditioned, no clip is handed back) and the network on their exact kernels;
 *   kws_run_classifier_batch_device and kws_extract_mfcc_batch_device follow the mode, the entry points that start from mel matrices
 *   (streams, kws_cmvn_inference_batch_device) have nothing left to relax.  That is the tuned MFE shape (fft 256, 32 or 40 filters, at most
 *   51 frames -- 52 up to 16 filters --, a window of at least 17 / 13 rows, 16-byte aligned frames); an MFE block at any other shape the
 *   general MFCC path accepts (below) runs on the general kernels, exact mode only: kws_set_mode(KWS_MODE_FAST) returns
 *   KWS_ERROR_UNSUPPORTED_MODEL with the reason, as for a general MFCC plan. */
#define KWS_MODE_EXACT 0
#define KWS_MODE_FAST 1
EI_IMPULSE_ERROR kws_set_mode(kws_handle *h, int mode);   /* KWS_ERROR_UNSUPPORTED_MODEL if the model's DSP configuration is outside the fast kernel (general-shape kernels) */
int kws_get_mode(const kws_handle *h);
/* 1: KWS_MODE_FAST runs this model's network fused behind the MFCC block (float32 CONV_2D graphs); 0: features go through HBM */
int kws_fast_is_fused(const kws_handle *h);
/* Where the fused float32 plan keeps the weight fragments of its split-operand convolution blocks: bit b set = block b's fragments have a copy in the
 * workgroup's LDS block, clear = they are read from device memory (through L2) -- or block b is no such block.  0 for a model without a fused float32 plan. */
int kws_fast_lds_fragments(const kws_handle *h);
/* What the last KWS_MODE_FAST batch call on this handle did with its clips (both synchronise the device):
 *   kws_fast_fallback_count  clips the fast kernel (first tier) handed back.  They went to the SECOND tier: cepstra from the exact kernels
 *                            (bit-identical to the reference's), then the fast cmvnw + network from those -- about 0.4 x the exact path;
 *   kws_fast_exact_count     clips the second tier handed back in turn: they were finished by the exact kernels and carry the exact
 *                            mode's bits.
 * A float32 graph whose gain leaves the fast DSP tiers no room (entry_tier >= 2) takes another route since round 5: EVERY clip's feature
 * matrix comes from the exact kernels (bit for bit) and the fused network runs from it on the matrix cores; what is left to guard is the
 * network's own arithmetic against the clip's own scores.  Both counts then are the (normally zero) clips that guard sent through the
 * exact network as well.
 * When a tier hands a clip back -- the rule follows from the LOADED MODEL: cmvnw divides whatever the fast arithmetic
 * moved in a cepstral coefficient, or in a window's mean, by the window's deviation; the graph carries a feature error into its logits with
 * a gain that depends on its weights.  kws_create measures that gain per cepstral column (reverse differentiation of the float graph on a
 * calibration set: kws_fast_gain) and the kernels sum, per clip,
 *     V = sigma_net^2 + sum over cmvnw windows (row r, column c) of ((abs[c] + lev[c] x level + rel[c] x |window mean|) / (deviation + eps))^2
 * -- an estimate of the variance of the error of a logit difference; abs / lev / rel = gain[c] x the rms error of a coefficient (absolute,
 * per unit of the clip's log-mel level = mean over its frames of |mean over the filters of the log-mel energies|, per unit of |mean|:
 * kws_fast_guard), level = 0 for tier 2.  Tier 1, clips with digitally silent frames (kws_fast_tolerance::silent_rows_exact): those frames' rows are
 * the reference's own, so abs and lev are multiplied by sqrt(live frames / frames) and level is taken over the live frames.  The clip stays in its tier iff
 *     V x max(g_c1 x P^2, g_c2) <= 1,    g_c1 = (k_sigma x lin_margin / score_tol)^2,  g_c2 = (k_sigma / logit_cap)^2,
 * P = the largest p (1 - p) among the clip's own scores where the network runs in the same launch (|d score| <= p (1 - p) x the error of
 * a logit difference: a saturated softmax passes nothing on), 1/4 otherwise.  In words: k_sigma standard deviations of the estimated logit
 * error, through the clip's own softmax, must stay below the score tolerance of 1e-4.  A calibrated statistical estimate, not a bound
 * (a worst-case bound through the weights' row sums would refuse every model); tests/test_gpu_fast_families.py re-evaluates the rule
 * from the oracle's cepstra and holds scores AND logits to it on eleven input families.
 * How many standard deviations k_sigma is worth depends on how well the calibrated gain covers the clip at hand: gain[c] is the largest value
 * over 48 calibration matrices x 1.25.  On real clips' Jacobians (tests/test_gain_calibration.py) no clip's total gain exceeds the calibrated
 * one -- the full 4.5 sigma for an error spread over the columns -- and a single column's gain reaches at most 1.3 x the calibrated value:
 * 4.5 / 1.3 = 3.4 sigma for a clip whose whole error sat in that column (kws_fast_tolerance::k_sigma_worst_column).  For a graph whose
 * activation patterns on its real inputs differ from anything the calibration set reaches, nothing bounds the underestimate: the numbers
 * are what was measured on the shipped graphs.
 * int8 graphs have no float logits to protect (the network is bit-exact from its int8 input tensor on): gain[c] is the constant for which
 * the rule reads "k_sigma x the rms of the clip's feature error estimates <= 1e-4", calibrated = 0.
 *   kws_fast_guard   coef [4][n_columns]: abs, lev, rel, and the alternative rel: column 0 -- when its window means were replayed in the reference's
 *                    order (a decision of the kernel; always for a clip with digitally silent frames); the other columns -- where the reference's
 *                    sequential window sums round systematically: every column of a clip with digitally silent frames (a frame energy of exactly 0),
 *                    and (float32 graphs) a column whose deviation is below kws_fast_tolerance::systematic_ratio x |mean| in its lane's first window
 *   kws_fast_gain    gain [n_columns] of a float32 graph (logit-difference error per unit of feature error, rms over a column's rows)
 * kws_streams_step_device and kws_cmvn_inference_batch_device start from exact cepstra: their one fast tier is tier 2. */
typedef struct {
    float score_tol, k_sigma, lin_margin, logit_cap;   /* 1e-4, 4.5, 1.1, 0.1 */
    float g_c1, g_c2;                                  /* as above */
    float sigma_net;                                   /* sqrt of the clip-independent part of V: the matrix cores' summation order in a fused float32 graph, the
                                                          relative error of a window's deviation (x total_gain) */
    float total_gain;                                  /* sqrt(sum over all features of gain^2) */
    float uniform_feature_tol;                         /* the feature error of random sign, the same size on every feature, that exactly meets the rule at P = 1/4 */
    int calibrated, n_columns, n_frames;
    int entry_tier;                                    /* where kws_run_classifier_batch_device starts in KWS_MODE_FAST: 1 the fast kernel; 2 / 3: the graph's gain
                                                          leaves tier 1 (and tier 2) no room -- a typical clip would be handed on anyway.  float32 graphs of the
                                                          fused shapes then get the exact kernels' feature matrix + the network on the matrix cores; other graphs:
                                                          2 = exact cepstra for every clip, then the fast cmvnw + network; 3 = the exact kernels.  Routing only:
                                                          every tier applies its guard */
    int dev_overrides;                                 /* non-zero: a KWS_DEV_FAST_* development switch (guard off / scaled, no re-run) was set in the environment when
                                                          the model was created -- KWS_MODE_FAST results are then outside the documented tolerance */
    float k_sigma_worst_column;                        /* k_sigma / 1.3: what k_sigma is worth for a clip whose whole error sits in the column where a real clip's gain was
                                                          measured furthest above the calibrated one (see above); = k_sigma for int8 graphs (no gain is calibrated) */
    int silent_rows_exact;                             /* 1 (round 6): the rows of digitally silent frames (frame energy exactly 0) carry the reference's own cepstral
                                                          row in tier 1 -- recorded at kws_create from the exact kernels on an all-zero window --, so the rule's abs / lev
                                                          terms are multiplied by sqrt(live frames / frames) and `level` is the mean over the LIVE frames only */
    float systematic_ratio;                            /* a column whose deviation is below this x |mean| in a lane's first window (rows 0, cr, 2 cr ... of the kernel's
                                                          row groups, cr = 13 for up to 16 columns and in the three-waves-per-SIMD build, else 17) takes the alternative rel coefficient, like a clip with silent frames (column 0 of
                                                          such a clip always has its window means replayed) */
    int fused_waves_per_simd, fused_waves;             /* (round 6) the build of the fast kernel a float32 graph's batch calls enter through: 2 waves per SIMD (8 per
                                                          workgroup, 256 registers) or 3 (12 / 11 per workgroup, <= 168 registers, clips dealt out by ticket: plans that
                                                          enter through the PCM form and hold at least eleven waves in the LDS block); 0, 0: no fused float32 form */
} kws_fast_tolerance;
EI_IMPULSE_ERROR kws_fast_fallback_count(kws_handle *h, size_t *count);
EI_IMPULSE_ERROR kws_fast_exact_count(kws_handle *h, size_t *count);
EI_IMPULSE_ERROR kws_fast_guard(const kws_handle *h, int tier, float *coef);
EI_IMPULSE_ERROR kws_fast_gain(const kws_handle *h, float *gain);
EI_IMPULSE_ERROR kws_fast_tolerance_info(const kws_handle *h, kws_fast_tolerance *out);

/* float32 graphs: the device-resident batch entry points that produce scores (kws_run_classifier_batch_device,
 * kws_cmvn_inference_batch_device) also write every clip's FULLY_CONNECTED outputs -- the logits the SOFTMAX reads -- to
 * logits [B][label_count] (device) until the tap is cleared with NULL; both modes, every tier of KWS_MODE_FAST.  A score near 0 or 1 hides
 * its logit (d score = p (1 - p) d logit): the parity tests of the fast mode hold the logits themselves.  B is the calling batch's. */
EI_IMPULSE_ERROR kws_set_logits_tap(kws_handle *h, float *logits);

/* The model used by the SDK-style entry points run_classifier()/run_inference().  If none was set,
 * the first call loads the file named by the environment variable KWS_MODEL on device KWS_DEVICE (0). */
EI_IMPULSE_ERROR kws_set_default_model(kws_handle *h);
kws_handle *kws_default_model(void);

/* ---- the hot path, batch form: replaces run_classifier() for B clips ------------------------------
 * pcm      [B][clip_samples] int16, device
 * scores   [B][label_count]  float, device  (classification[].value of each clip)
 * features [B][feature_count] float, device, optional (NULL to skip): extract_mfcc_features output
 * q_in     [B][feature_count] int8,  device, optional: the quantised input tensor              */
EI_IMPULSE_ERROR kws_run_classifier_batch_device(kws_handle *h, const int16_t *pcm, size_t B, float *scores,
                                                 float *features, int8_t *q_in, void *stream);
/* host pointers; copies in, runs, copies out, synchronises */
EI_IMPULSE_ERROR kws_run_classifier_batch(kws_handle *h, const int16_t *pcm, size_t B, float *scores,
                                          float *features, int8_t *q_in);

/* ---- the stages, for callers that hold intermediate data already and for parity tests ------------- */
/* speechpy::feature::mfcc for B windows (dsp/speechpy/feature.hpp:370-439): cepstra BEFORE cmvnw,
 * mfcc [B][feature_count] float, device */
EI_IMPULSE_ERROR kws_mfcc_batch_device(kws_handle *h, const int16_t *pcm, size_t B, float *mfcc, void *stream);
/* processing::cmvnw (processing.hpp:326-389) + run_inference (ei_run_classifier.h:293-493) on B cepstral
 * matrices; features / q_in optional outputs as above */
EI_IMPULSE_ERROR kws_cmvn_inference_batch_device(kws_handle *h, const float *mfcc, size_t B, float *scores,
                                                 float *features, int8_t *q_in, void *stream);
/* speechpy::feature::mfe for B clips (dsp/speechpy/feature.hpp:193-318; the MFE block's front end):
 * mel [B][frames][filters] filterbank energies and energy [B][frames] frame energies (may be NULL), both after
 * zero handling, before any log. */
EI_IMPULSE_ERROR kws_mfe_batch_device(kws_handle *h, const int16_t *pcm, size_t B, float *mel, float *energy, void *stream);
/* extract_mfe_features for B clips -- the MFE DSP block of the newer SDK copy (nucleo-l432 .../edge-impulse-sdk/classifier/
 * ei_run_dsp.h:369-418): speechpy::feature::mfe on the raw signal (no pre-emphasis), processing::cmvnw(win_size, false, true)
 * (dsp/speechpy/processing.hpp:327-399) and numpy::normalize (dsp/numpy.hpp:1391-1429).  Frame / filter / window settings are
 * the model's DSP settings; features [B][frames * filters] float, device.
 * Shapes: every DSP configuration kws_create accepts -- for an MFE-block model that is what a general MFCC plan meets with columns = filters:
 * an even fft_length whose half factors into 2, 3, 4, 5 (128 ... 2048), an even filter count of 32 to 128 whose half factors likewise (fewer than 32 filters: the tuned shape only), an odd
 * win_size, any frame count, stride and window length, frames x filters == the network's input size.  The tuned shape keeps its kernels; the
 * others run the general spectral kernels (the tuned one over chunks of frames where fft 256, 32 / 40 filters and 16-byte aligned frames
 * allow it) and a normalisation kernel that keeps a clip's padded matrix in LDS -- or, past 64 KB, works through global memory: no shape is
 * refused for its size.  A constant clip (range 0) comes out as the reference's 0 x inf NaNs.  (Called on an MFCC-block model, the call
 * normalises in place in `features` and refuses the few shapes whose padded matrix exceeds the LDS form.) */
EI_IMPULSE_ERROR kws_extract_mfe_batch_device(kws_handle *h, const int16_t *pcm, size_t B, float *features, void *stream);
/* extract_mfcc_features for B clips (classifier/ei_run_dsp.h:256-308) */
EI_IMPULSE_ERROR kws_extract_mfcc_batch_device(kws_handle *h, const int16_t *pcm, size_t B, float *features,
                                               int8_t *q_in, void *stream);
/* run_inference for B feature vectors (ei_run_classifier.h:293-493) */
EI_IMPULSE_ERROR kws_run_inference_batch_device(kws_handle *h, const float *features, size_t B, float *scores,
                                                void *stream);
/* network only, from int8 input tensors; optional int8 taps (device, may be NULL):
 *   tap_pooled [B][kws_pooled_tap_bytes]  every MAX_POOL_2D output, in graph order; behind them the int8 output of every hidden
 *                                         FULLY_CONNECTED layer of a dense stack, in graph order
 *   tap_fc     [B][label_count]           output of the (last) FULLY_CONNECTED
 *   tap_out    [B][label_count]           SOFTMAX output                                         */
EI_IMPULSE_ERROR kws_nn_batch_device(kws_handle *h, const int8_t *q_in, size_t B, float *scores, int8_t *tap_pooled,
                                     int8_t *tap_fc, int8_t *tap_out, void *stream);
EI_IMPULSE_ERROR kws_nn_batch(kws_handle *h, const int8_t *q_in, size_t B, float *scores, int8_t *tap_pooled,
                              int8_t *tap_fc, int8_t *tap_out);
/* float32 models (the reference's float kernels: TFL/kernels/internal/reference/conv.h:28-99, add.h:179-215,
 * pooling.h:189-237, fully_connected.h:26-60, softmax.h:31-63): network only, from float feature vectors; optional tap
 *   tap_logits [B][label_count]  FULLY_CONNECTED output (bit-identical to the reference; softmax uses the device expf).
 * The int8 entry points above return KWS_ERROR_UNSUPPORTED_MODEL for a float model, and this one for an int8 model;
 * kws_run_classifier_batch*, kws_run_inference_batch_device, kws_cmvn_inference_batch_device, the stream API and the
 * SDK entry points serve both kinds (int8 outputs must then be NULL). */
EI_IMPULSE_ERROR kws_nn_f32_batch_device(kws_handle *h, const float *features, size_t B, float *scores,
                                         float *tap_logits, void *stream);

/* ---- continuous mode for S streams in lock step ----------------------------------------------------
 * Each stream follows run_classifier_continuous() (classifier/ei_run_classifier.h:184-282): one slice of audio per
 * step, a rolling cepstra buffer, whole-window cmvnw + network once it is full, 2-tap moving average per class
 * (ei_run_classifier.h:134-145).  All per-stream state lives in HBM.  As in the reference, every step of a batch
 * but its very first claims one extra frame length (ei_run_dsp.h:319-325; not reset by kws_streams_init) and
 * pre-emphasis then needs the sample one frame beyond the slice: pass those S floats in end_of_signal (device),
 * or NULL for 0 (what the reference sees when the application's get_data refuses the read).
 *   slices [S][slice_samples] int16 (device), scores [S][label_count] float (device), *produced = inference ran. */
typedef struct kws_stream_batch kws_stream_batch;
EI_IMPULSE_ERROR kws_streams_create(kws_handle *h, size_t S, kws_stream_batch **out);
void kws_streams_destroy(kws_stream_batch *sb);
EI_IMPULSE_ERROR kws_streams_init(kws_stream_batch *sb);            /* run_classifier_init, ei_run_classifier.h:164 */
EI_IMPULSE_ERROR kws_streams_step_device(kws_stream_batch *sb, const int16_t *slices, size_t slice_samples,
                                         const float *end_of_signal, float *scores, int *produced, void *stream);

/* ---- continuous mode over whole recordings: every window of R recordings in one call ---------------------------------
 * Parity contract.  For each recording r, the call returns exactly what a NEWLY CREATED kws_stream_batch with S = 1 returns when it is
 * stepped through the recording with kws_streams_step_device:
 *   - the recording is consumed as floor(lengths[r] / slice_samples) consecutive slices; a trailing partial slice is ignored;
 *   - every recording starts from fresh state (first_run false, zero feature buffer, zero moving-average filters); the process-global
 *     first_run of the reference is NOT carried from one recording to the next;
 *   - slice k is the signal_t whose get_data(offset, n) reads the recording from sample k * slice_samples + offset: a read inside the
 *     recording returns those samples, converted like every other sample of the slice (x / 32768); a read past the recording's end fails,
 *     so the reference's pre-zeroed buffer gives 0.  In practice this concerns only the pre-emphasis x[-1] of the slices k >= 1, the
 *     sample at k * slice_samples + slice_samples + frame_length - 1 (the stream API's end_of_signal);
 *   - window w of the recording is produced at the step where kws_streams_step_device reports *produced (with the shipped slicing,
 *     4000-sample slices of a 16 000-sample window: the fourth slice and every later one, W = n_slices - 3), and carries that step's scores.
 * Window counts: kws_scan_window_count (host arithmetic only).  Recording r's windows are rows [sum_{q<r} W_q, + W_r) of the outputs.
 *   pcm         int16, device; recording r is lengths[r] samples at pcm + offsets[r] (any sample offset, no alignment needed)
 *   offsets, lengths  [R], HOST arrays
 *   scores      [sum_r W_r][label_count] float, device: what run_classifier_continuous returns (after the moving average)
 *   raw_scores  [sum_r W_r][label_count] float, device, optional (NULL): the same windows before the moving average
 * Slicings and models: exactly what kws_streams_step_device accepts (int8, float32 and MFE-block models -- tuned or general shape --, general-shape DSP
 * configurations); a slicing that the stream API refuses at any step is refused with the same error code, whatever the lengths.
 * R = 0, or no recording long enough for a window: EI_IMPULSE_OK, nothing written.  scores == NULL: KWS_ERROR_BAD_ARGUMENT.
 * Mode: KWS_MODE_EXACT is bit-identical to the stream API; KWS_MODE_FAST follows its rule (exact slice cepstra, then the fast cmvnw +
 * network behind the guard; windows the guard hands back are re-run by the exact kernels inside the call), and kws_fast_fallback_count /
 * kws_fast_exact_count report the windows of the last scan call that were handed back.  Scan calls do not write the logits tap.
 * Device memory: the call keeps (on the handle, grown on demand; growing synchronises the device) the cepstral rows of its recordings --
 * about (n_slices x frames per slice x columns) floats per recording, the only part that grows with the audio -- plus bounded scratch:
 * at most 32 MiB of staged slices and 64 MiB of windows gathered for the network (chunks of at most 32 768 windows), 32 bytes per
 * recording and the handle's batch scratch for one chunk.  Ordering: as for every call on the handle (see the top of this file); the
 * call waits for earlier work on `stream` before it uploads its per-recording tables, the rest is asynchronous. */
EI_IMPULSE_ERROR kws_scan_window_count(const kws_handle *h, size_t n_samples, size_t slice_samples, size_t *n_windows);
EI_IMPULSE_ERROR kws_scan_recordings_device(kws_handle *h, const int16_t *pcm, const size_t *offsets, const size_t *lengths, size_t R,
                                            size_t slice_samples, float *scores, float *raw_scores, void *stream);

/* ---- one-shot windows over whole recordings: run_classifier() at every position, one window every hop_samples ---------------------
 * Parity contract.  Let clip = kws_clip_samples(h).  Recording r has W_r = lengths[r] < clip ? 0 : (lengths[r] - clip) / hop_samples + 1
 * windows (kws_slide_window_count; host arithmetic only); window w is samples [w hop_samples, w hop_samples + clip) of the recording.
 * Its row of `scores` is what kws_run_classifier_batch_device returns for that window copied out as a clip, and its row of `features`
 * likewise, in the handle's mode, whichever path runs and whatever `flags` says: in KWS_MODE_EXACT bit-identical to that call and, per
 * window, to the reference's run_classifier().  These are the ONE-SHOT features the models were trained on -- not continuous mode's
 * (kws_scan_*, kws_live_*: fake first frame, rows never written, cmvnw over a rolling buffer) -- and there is no moving average.
 * Recording r's windows are rows [sum_{q<r} W_q, + W_r) of the outputs.
 *   pcm         int16, device; recording r is lengths[r] samples at pcm + offsets[r] (any sample offset, no alignment needed)
 *   offsets, lengths  [R], HOST arrays
 *   scores      [sum_r W_r][label_count] float, device
 *   features    [sum_r W_r][feature_count] float, device, optional (NULL)
 *   flags       KWS_SLIDE_AUTO, or one path by name.  DIRECT: every window staged as a clip and its frame_count rows computed for it.
 *               SHARED: only a window's first sample takes its pre-emphasis predecessor from the window (its last sample), so frame
 *               f >= 1 of a window is the cepstral row of that position of the recording whichever window reads it: those rows are
 *               computed once per recording and position (hop_samples / gcd(hop_samples, frame stride) new rows per window), frame 0 once
 *               per window (MFE block: no pre-emphasis, frame 0 is shared too).  Both run the one-shot path's own spectral kernels and the
 *               same cmvnw + network launches: the paths are bit-identical to each other in either mode.
 *               AUTO takes SHARED where rows_shared + rows_first < rows_direct (kws_slide_plan reports all three, and the path).
 * Models: those of the scan (int8, float32 and MFE-block graphs, general-shape DSP configurations, MFE blocks among them).
 * hop_samples == 0, scores == NULL, unknown flags, a recording, offset or hop beyond 2^56 samples: KWS_ERROR_BAD_ARGUMENT.  R = 0, or no
 * recording long enough for a window: EI_IMPULSE_OK, nothing written.
 * Mode: KWS_MODE_EXACT as above; KWS_MODE_FAST follows the scan's rule (exact cepstral rows, then the fast cmvnw + network behind the
 * guard; windows the guard hands back are re-run by the exact kernels inside the call: scores within the fast mode's tolerance of the
 * exact ones), and kws_fast_fallback_count / kws_fast_exact_count report the windows of the last slide call that were handed back.
 * Slide calls do not write the logits tap.
 * Device memory: the call keeps (on the handle, grown on demand; growing synchronises the device) bounded scratch -- at most 32 MiB of
 * staged samples, 64 MiB of windows gathered for the network (chunks of at most 32 768 windows), one frame-0 row per window of a chunk,
 * the handle's batch scratch for one chunk -- plus, on the shared path only, the part that grows with the audio: the cepstral rows of the
 * call's recordings, about (lengths[r] / gcd(hop_samples, frame stride)) rows of feature_count / frame_count floats per recording
 * (3 000 rows = 156 KB per minute for the shipped models at a hop that is a multiple of the frame stride), and 24 bytes per recording
 * and phase.  Ordering: as for every call on the handle (see the top of this file); the call waits for earlier work on `stream` before
 * it uploads its tables, the rest is asynchronous. */
int kws_frame_stride_samples(const kws_handle *h);           /* the DSP block's frame stride in samples */
#define KWS_SLIDE_AUTO   0   /* the library picks the path */
#define KWS_SLIDE_DIRECT 1   /* every window's rows computed for that window */
#define KWS_SLIDE_SHARED 2   /* rows computed once per recording and position, frame 0 per window */
typedef struct {
    size_t n_windows;        /* sum over the recordings */
    size_t rows_shared;      /* cepstral rows the shared path computes once per position (items are padded to whole launches on top) */
    size_t rows_first;       /* per-window frame-0 rows (0 for an MFE block) */
    size_t rows_direct;      /* n_windows * frame_count: what the direct path computes */
    int    phases;           /* frame_stride / gcd(hop, frame_stride) */
    int    path;             /* KWS_SLIDE_DIRECT or KWS_SLIDE_SHARED: what a call with these arguments runs */
} kws_slide_plan_info;
EI_IMPULSE_ERROR kws_slide_window_count(const kws_handle *h, size_t n_samples, size_t hop_samples, size_t *n_windows);
EI_IMPULSE_ERROR kws_slide_plan(const kws_handle *h, const size_t *lengths, size_t R, size_t hop_samples, int flags,
                                kws_slide_plan_info *out);                                   /* host arithmetic only */
EI_IMPULSE_ERROR kws_slide_recordings_device(kws_handle *h, const int16_t *pcm, const size_t *offsets, const size_t *lengths, size_t R,
                                             size_t hop_samples, int flags, float *scores, float *features, void *stream);

/* ---- banks: K models that share one DSP block, scored in one call; the DSP block runs once -----------------------------------------
 * A bank is K model handles with an identical DSP block.  A bank call computes the front end once -- the feature matrix, from clips,
 * from cepstra or from the windows of whole recordings -- and every member's scores from it: an int8 graph next to its float32 twin,
 * a 2-conv graph next to a DS-CNN, one tenant's keyword set next to another's.
 * Membership.  1 <= K <= 16 handles on one device, none of them twice, equal in: DSP block kind (MFCC / MFE), every field of the DSP
 * configuration (axes, num_cepstral, frame_length, frame_stride, num_filters, fft_length, win_size, low_frequency, high_frequency,
 * pre_cof, pre_shift), sampling frequency, raw_sample_count and EIDSP_QUANTIZE_FILTERBANK -- so frames, columns and feature_count are
 * equal too.  int8 and float32 graphs, tuned and general-shape plans, MFCC and MFE blocks all qualify; label counts may differ.
 * Anything else: KWS_ERROR_BAD_ARGUMENT, kws_last_error names the first differing field.  kws_bank_create changes no member; a member
 * stays usable on its own; destroy banks before their members (kws_bank_destroy waits for the bank's enqueued work).
 * Parity contract.  Member k's rows of scores[k] are bit-identical to what kws_run_classifier_batch_device,
 * kws_cmvn_inference_batch_device or kws_slide_recordings_device writes for that member alone in KWS_MODE_EXACT on the same input, for
 * int8 and float32 graphs alike, and `features` is bit-identical to any member's own: int8 scores and features bit-exact with the
 * reference, float32 scores within 1e-6.  The slide's paths (AUTO, DIRECT, SHARED) stay bit-identical to each other.
 *   scores    HOST array of K DEVICE pointers; scores[k] is [rows][kws_label_count(member k)] float, or NULL to skip member k in this call
 *   features  [rows][feature_count] float, device, optional (NULL): the shared feature matrix
 *   rows      B; for the slide sum_r W_r -- window counts (kws_slide_window_count) and kws_slide_plan are any member's
 *   other arguments as in the single-model entry point of the same name
 * Mode.  Bank calls always run the exact kernels, like the host-buffer entry point: they neither read nor change the members'
 * kws_set_mode state, fast counters (kws_fast_fallback_count / kws_fast_exact_count) or logits taps, and write no tap.
 * B = 0, or no recording long enough for a window: EI_IMPULSE_OK, nothing written.  Every scores[k] NULL and features NULL, a NULL
 * bank, pcm / mfcc or scores array, B >= 2^31, and whatever kws_slide_recordings_device refuses: KWS_ERROR_BAD_ARGUMENT.
 * Ordering.  A bank call counts as a call on EVERY member handle for the rules at the top of this file (a call on another stream than a
 * member's previous call first waits for that call); it holds the members' locks for its duration, taken in one fixed order (by
 * address) whatever the members' order, so banks over the same handles cannot deadlock.  Calls on one bank are serialised.
 * Device memory.  The bank owns K records of 1 072 bytes (the int8 members' plans, written once) and, for calls without `features`, the shared
 * feature matrix: B x feature_count floats (the slide: one chunk, at most 64 MiB), grown on demand; growing synchronises the device.
 * int8 members outside the two-block matrix-core shape take their input tensor from their own batch scratch (grown to B clips: 5 bytes
 * per feature value, as for their own calls); the slide reuses the FIRST member's slide scratch, with kws_slide_recordings_device's
 * bounds, and that member's batch scratch for one chunk. */
typedef struct kws_bank kws_bank;
EI_IMPULSE_ERROR kws_bank_create(kws_handle *const *members, size_t K, kws_bank **out);
void kws_bank_destroy(kws_bank *b);
size_t kws_bank_size(const kws_bank *b);
kws_handle *kws_bank_member(const kws_bank *b, size_t k);                  /* NULL for k >= K */
/* run_classifier() for B clips and K models: the DSP block once, every member's network from its output */
EI_IMPULSE_ERROR kws_bank_run_classifier_batch_device(kws_bank *b, const int16_t *pcm, size_t B, float *const *scores, float *features,
                                                      void *stream);
/* the same from cepstra before cmvnw (kws_mfcc_batch_device of any member): cmvnw / the MFE normalisation once */
EI_IMPULSE_ERROR kws_bank_cmvn_inference_batch_device(kws_bank *b, const float *mfcc, size_t B, float *const *scores, float *features,
                                                      void *stream);
/* kws_slide_recordings_device for K models: staging, cepstral rows, gathering and cmvnw once per window */
EI_IMPULSE_ERROR kws_bank_slide_recordings_device(kws_bank *b, const int16_t *pcm, const size_t *offsets, const size_t *lengths, size_t R,
                                                  size_t hop_samples, int flags, float *const *scores, float *features, void *stream);

/* ---- clips of their own lengths: run_classifier() for B clips, each as long as it is, in one call -----------------------------------
 * run_classifier() accepts a window of any length that yields 1 .. kws_frame_count(h) frames (the shipped impulse: 640 .. 16 319 samples)
 * and classifies it from the frames that fit: they are normalised among themselves, x[-1] is the last sample of THAT window, and the
 * rest of the network's input stays at the zeros of the reference's calloc'd matrix.  kws_run_classifier_ragged_device does that for a
 * batch of isolated utterances -- speech-commands style files, the segments a VAD cuts out -- without padding them (padding changes the
 * window the model sees: another wrap sample, other cmvnw statistics).  Clip i is lengths[i] samples at pcm + offsets[i].
 * Parity contract.  Row i of `scores` is what run_classifier() returns for a signal_t of total_length = lengths[i] over those samples.
 * Row i of `features` ([feature_count]) holds extract_mfcc_features / extract_mfe_features of the frames that fit in its first
 * frames x columns values (kws_window_frame_count(h, lengths[i]) frames; columns: cepstra, or mel filters for an MFE block), and every
 * later value of the row is +0.0f -- the call WRITES them, the caller's buffer is not assumed clean.  Row i of `q_in` is run_inference's
 * quantisation of that whole matrix.  A clip with lengths[i] == kws_clip_samples(h) gets exactly the bits
 * kws_run_classifier_batch_device gives it in KWS_MODE_EXACT.  int8 graphs: bit-exact with the reference; float32 graphs: features and
 * logits bit-exact, scores within 1e-6 (the bars of the other entry points).
 *   pcm       DEVICE pointer, int16
 *   offsets   HOST array [B], in samples from pcm: any value, no alignment needed; clips may overlap or repeat
 *   lengths   HOST array [B], in samples
 *   scores    [B][label_count] float, device, or NULL: the network is skipped (a ragged extract_mfcc_features / extract_mfe_features)
 *   features  [B][feature_count] float, device, optional (NULL)
 *   q_in      [B][feature_count] int8, device, optional (NULL); KWS_ERROR_UNSUPPORTED_MODEL for a float32 graph, as in the batch call
 * The call reads no sample outside [offsets[i], offsets[i] + lengths[i]) for any i: what lies between and around the clips does not
 * matter and need not be mapped.
 * Lengths.  Every clip must have 1 .. kws_frame_count(h) frames.  The lengths are checked on the host before anything is enqueued: one bad
 * clip refuses the whole call with KWS_ERROR_BAD_ARGUMENT, kws_last_error names the first offending index and its length, nothing is
 * written.  Longer audio is kws_slide_recordings_device's job (one window every hop); this call does not cut recordings.  Also
 * KWS_ERROR_BAD_ARGUMENT: scores, features and q_in all NULL; B >= 2^31; NULL pcm / offsets / lengths with B > 0.  B == 0: EI_IMPULSE_OK,
 * nothing written.
 * Mode.  The call always runs the exact kernels, like bank calls: it neither reads nor changes kws_set_mode state, the fast counters
 * (kws_fast_fallback_count / kws_fast_exact_count) or the logits tap, and writes no tap.
 * Models.  Everything the batch call serves: int8 and float32 graphs, MFCC and MFE blocks, tuned and general-shape DSP plans (either block).
 *   MFCC block on the tuned shapes (fft 256, 32 or 40 filters): the whole DSP block of the batch is ONE launch, however many distinct
 *     lengths it holds (the ragged form of kws_mfcc8_kernel: frame count, length, base address and pad map per clip).  A clip whose first
 *     sample lies on a 16-byte boundary (pcm 16-byte aligned, offset a multiple of 8 samples) is read in place, no copy of its audio is
 *     made; the others are first copied into aligned slots of a staging buffer by one more launch.
 *   MFE blocks and general-shape plans take a grouped route: the clips are bucketed by frame count on the host and every bucket goes
 *     through the fixed-length launches with the plan of its frame count (gathered into slots of one stride, scattered into the
 *     full-stride rows): a handful of launches per DISTINCT frame count in the batch.
 * Device memory, ordering, streams.  As for the other calls on a handle (top of this file): a call on another stream than the handle's
 * previous call first waits for it.  Scratch is on the handle, grown on demand; growing synchronises the device.  The call keeps: the
 * per-clip descriptor table (16 bytes per clip; as much again for the clips that are staged or gathered), the pad maps of all row counts
 * (uploaded once per handle), the handle's batch scratch for B clips where the network's input is not handed out, and a staging buffer
 * only for the clips that need one -- tuned shapes: the clips not on a 16-byte boundary, in slots of the longest of them; grouped route:
 * the largest bucket, plus its packed feature rows. */
/* frames the reference's framing yields for a window of n_samples (processing.hpp:194-284); 0: none fits (or h is NULL) */
int kws_window_frame_count(const kws_handle *h, size_t n_samples);
EI_IMPULSE_ERROR kws_run_classifier_ragged_device(kws_handle *h, const int16_t *pcm, const size_t *offsets, const size_t *lengths,
                                                  size_t B, float *scores, float *features, int8_t *q_in, void *stream);

/* ---- live continuous mode: audio of any length pushed to any subset of S streams, state in HBM between calls ----------------------
 * A session holds S streams at one slicing.  A push hands any number of new samples (0 included) to any subset of the streams, each its
 * own length, and returns every window those samples complete; finishing a stream flushes what waited for its look-ahead sample and the
 * stream starts over from fresh state.
 * Parity contract.  Take the concatenation of everything pushed to a stream since it was created, reset or last finished, up to and
 * including the push that finishes it.  The windows the pushes return for that stream, in order, are exactly the windows
 * kws_scan_recordings_device returns for that concatenation as one recording at the same slice_samples (scores and raw_scores; in
 * KWS_MODE_EXACT bit-identical).  Before the stream is finished, the windows returned so far are the scan's first windows of the whole
 * recording: a slice k >= 1 reads its look-ahead sample (k * slice_samples + slice_samples + frame_length - 1), so a push holds such a
 * slice back, and every window that ends in it, until that sample has arrived; only a finish reads it as 0 past the end.
 *   kws_live_create   S streams (0 < S < 2^30) at slice_samples; a slicing the stream API refuses is refused with kws_scan_window_count's
 *                     code.  Models: those of the scan (int8, float32, MFE-block graphs, general-shape DSP configurations).
 *   kws_live_destroy  waits for the session's enqueued work, then frees it.  Destroy sessions before their handle.
 *   kws_live_reset    streams [n] (HOST; NULL: all): back to fresh state, as if just created.  Host only: no device work.
 *   kws_live_window_count  the windows a push of n_new samples (finish != 0: and finishing) to `stream` would return now (host only)
 *   kws_live_push_device  n entries; streams, offsets, lengths, finish (NULL: none finishes) and n_windows are HOST arrays of n entries.
 *                     Entry i hands lengths[i] samples at pcm + offsets[i] (int16, device, any sample offset) to stream streams[i]; entry i's
 *                     windows are rows [sum_{j<i} n_windows[j], + n_windows[i]) of scores / raw_scores ([.][label_count] float, device;
 *                     raw_scores optional: before the moving average).  n_windows is computed on the host before anything is launched
 *                     (the session keeps host copies of every stream's sample and slice counts); the call reads nothing back.
 * Streams not named in a push keep their state.  KWS_ERROR_BAD_ARGUMENT, with no state changed: a stream named twice in one push, a stream
 * index >= S, n > 0 with streams, lengths, n_windows or scores NULL, samples pushed with pcm or offsets NULL, more than 2^60 samples to one
 * stream between starts.  A push with no window writes nothing to scores.  If a push fails past its argument checks, reset the streams
 * it named.
 * Mode follows the handle at push time, as in the scan: KWS_MODE_FAST runs the exact slice cepstra, then the fast cmvnw + network behind
 * the guard, with windows it hands back re-run inside the call; kws_fast_fallback_count / kws_fast_exact_count report the windows of the
 * last push (0 for a push without windows).  Pushes write no logits tap.
 * Device memory per stream, bounded whatever the audio length: the carried samples, a ring of slice_samples + frame_length int16
 * (8 640 B at the shipped slicing); the last ring_rows - frames per slice cepstral rows (35 x 13 floats = 1 820 B shipped); the moving
 * average's taps and running sum per label (3 floats per label).  On top, per session and grown on demand (growing synchronises the
 * device), the scan's per-call scratch: at most 32 MiB of staged slices, 64 MiB (<= 32 768) of gathered windows, the cepstral rows of
 * the slices one push finishes and 80 B per entry; plus the handle's batch scratch for one chunk of windows.  Ordering: as for every call
 * on the handle; a push waits for earlier work on `stream` before it uploads its per-entry tables, the rest is asynchronous. */
typedef struct kws_live kws_live;
EI_IMPULSE_ERROR kws_live_create(kws_handle *h, size_t S, size_t slice_samples, kws_live **out);
void kws_live_destroy(kws_live *lv);
EI_IMPULSE_ERROR kws_live_reset(kws_live *lv, const size_t *streams, size_t n);
EI_IMPULSE_ERROR kws_live_window_count(const kws_live *lv, size_t stream, size_t n_new, int finish, size_t *n_windows);
EI_IMPULSE_ERROR kws_live_push_device(kws_live *lv, size_t n, const size_t *streams, const int16_t *pcm, const size_t *offsets,
                                      const size_t *lengths, const int *finish, float *scores, float *raw_scores, size_t *n_windows,
                                      void *stream);

/* ---- live one-shot windows: audio of any length pushed to any subset of S streams, every hop's run_classifier() result ----------------
 * A session holds S streams at one hop.  A push hands any number of new samples (0 included) to any subset of the streams, each its own
 * length, and returns every one-shot window those samples complete: the slide (kws_slide_recordings_device) cut into pushes, with the
 * features the models were trained on -- not continuous mode's (kws_live_*).
 * Parity contract.  Let clip = kws_clip_samples(h); number a stream's samples from its start (its creation or last reset).  Window w is
 * samples [w hop_samples, w hop_samples + clip) and is complete once sample w hop_samples + clip - 1 has arrived: a one-shot window has no
 * look-ahead sample, so nothing is held back and there is no finish flag.  With windows(n) = n < clip ? 0 : (n - clip) / hop_samples + 1
 * (kws_slide_window_count), a push of lengths[i] samples to stream streams[i], which had n0 samples, returns the windows windows(n0) up to,
 * not including, windows(n0 + lengths[i]); entry i's windows are rows [sum_{j<i} n_windows[j], + n_windows[i]) of `scores` and of the
 * optional `features`.  Take everything pushed to a stream since its start as one recording: the rows the pushes return for that stream, in
 * order, are exactly the rows kws_slide_recordings_device returns for that recording at the same hop_samples -- scores and features, in the
 * handle's mode at push time, on whichever path the session runs.  In KWS_MODE_EXACT they are bit-identical to the slide's and so, through
 * the slide's contract, to kws_run_classifier_batch_device on the window cut out as a clip and to the reference's run_classifier().  In
 * KWS_MODE_FAST they are bit-identical to the fast slide's (every tier of the fast finishing step works per window), and
 * kws_fast_fallback_count / kws_fast_exact_count describe the last push (0 for a push without windows).  Pushes write no logits tap.
 * Streams not named in a push keep their state.  With hop_samples > clip the samples between two windows are dropped as they arrive.
 *   kws_slide_live_create   S streams (0 < S < 2^30) at hop_samples; flags are the slide's.  Models: those of the slide (int8 and float32
 *                     graphs, MFCC and MFE blocks, tuned and general-shape DSP plans).
 *                     KWS_SLIDE_DIRECT serves any hop: every completed window is staged as a clip from the stream's carried samples and
 *                     the pushed chunk, and its frame_count rows are computed for it.
 *                     KWS_SLIDE_SHARED, the retained-row path, serves hop_samples % frame stride == 0 with hop_samples / frame stride <=
 *                     frame_count - pre (pre = 1; 0 for an MFE block: no pre-emphasis): frame f >= pre of window w is the cepstral row of
 *                     position w hop_samples / stride + f of the stream, so a push computes only the positions its completed windows need
 *                     and no earlier push has computed, plus frame 0 of each completed window (its predecessor sample is the window's
 *                     last); the stream keeps its last frame_count - pre rows between pushes.
 *                     KWS_SLIDE_AUTO takes SHARED where it is served and computes fewer rows per window (hop_samples / stride + pre <
 *                     frame_count), else DIRECT -- the slide's rule, by row count.  Hops that are no multiple of the frame stride run
 *                     DIRECT (retained rows per phase: not in this version).  Both paths run the one-shot path's own spectral kernels
 *                     and the same finishing launches: bit-identical to each other in either mode.
 *   kws_slide_live_destroy  waits for the session's enqueued work, then frees it.  Destroy sessions before their handle.
 *   kws_slide_live_path     KWS_SLIDE_DIRECT or KWS_SLIDE_SHARED: what the session's pushes run
 *   kws_slide_live_reset    streams [n] (HOST; NULL: all): back to fresh state, as if just created.  Host only: no device work.
 *   kws_slide_live_window_count  the windows a push of n_new samples to `stream` would return now (host only)
 *   kws_slide_live_push_device   n entries; streams, offsets, lengths and n_windows are HOST arrays of n entries.  Entry i hands lengths[i]
 *                     samples at pcm + offsets[i] (int16, device, any sample offset) to stream streams[i].  scores [.][label_count] float,
 *                     device; features [.][feature_count] float, device, optional (NULL).  n_windows is computed on the host before
 *                     anything is launched (the session keeps host copies of every stream's sample and computed-row counts); the call
 *                     reads nothing back.
 * KWS_ERROR_BAD_ARGUMENT, with no state changed and nothing written: S == 0 or S >= 2^30; hop_samples == 0 or beyond the slide's limit;
 * unknown flags; KWS_SLIDE_SHARED at a hop the retained-row path does not serve; a stream named twice in one push, a stream index >= S;
 * n > 0 with streams, lengths, n_windows or scores NULL; samples pushed with pcm or offsets NULL; more than 2^60 samples to one stream
 * between starts.  A push that completes no window writes nothing to scores / features.  If a push fails past its argument checks, reset
 * the streams it named.
 * Device memory per stream, bounded whatever the audio length: the carried samples -- from the next incomplete window's start on, fewer
 * than clip -- in a ring of clip int16 (32 000 B for the shipped models); on the shared path the last frame_count - pre cepstral rows
 * (48 x 13 floats = 2 496 B, 48 x 40 floats = 7 680 B shipped).  On top, per session and grown on demand (growing synchronises the
 * device), the slide's per-call scratch: at most 32 MiB of staged samples, 64 MiB (<= 32 768) of gathered windows, the cepstral rows one
 * push computes and 72 B per entry; plus the handle's batch scratch for one chunk of windows.  A session keeps nothing in the handle's
 * slide scratch: sessions at different hops and slide calls may interleave on one handle.  Ordering: a push counts as a call on the
 * handle (see the top of this file); it waits for earlier work on `stream` before it uploads its per-entry tables, the rest is
 * asynchronous. */
typedef struct kws_slide_live kws_slide_live;
EI_IMPULSE_ERROR kws_slide_live_create(kws_handle *h, size_t S, size_t hop_samples, int flags, kws_slide_live **out);
void kws_slide_live_destroy(kws_slide_live *sl);
int kws_slide_live_path(const kws_slide_live *sl);
EI_IMPULSE_ERROR kws_slide_live_reset(kws_slide_live *sl, const size_t *streams, size_t n);
EI_IMPULSE_ERROR kws_slide_live_window_count(const kws_slide_live *sl, size_t stream, size_t n_new, size_t *n_windows);
EI_IMPULSE_ERROR kws_slide_live_push_device(kws_slide_live *sl, size_t n, const size_t *streams, const int16_t *pcm, const size_t *offsets,
                                            const size_t *lengths, float *scores, float *features, size_t *n_windows, void *stream);

/* ---- banks over recording scans, live streams and clips of their own lengths --------------------------------------------------------
 * The bank forms of kws_scan_recordings_device, kws_live_*, kws_slide_live_* and kws_run_classifier_ragged_device: with these every entry
 * point that takes int16 audio has one.  Staging, the spectral kernels, gathering, cmvnw and -- in a live session -- every stream's
 * carried samples and retained rows exist ONCE, through the first member; each member adds its network, and in continuous mode its
 * moving-average filters, which one kernel launch serves for all members.
 *   scores, raw_scores   HOST arrays of K DEVICE pointers, as in the bank calls above; scores[k] is [rows][kws_label_count(member k)] float
 *   features             [rows][feature_count] float, device, optional (NULL): the shared feature matrix (live slide, ragged)
 *   rows, n_windows      window counts are any member's (kws_scan_window_count, kws_*_live_window_count); the ragged call: rows = B
 *   other arguments as in the single-model entry point of the same name
 * Parity contract.  Member k's rows are bit-identical to what that member's own entry point writes in KWS_MODE_EXACT on the same input --
 * kws_scan_recordings_device, kws_live_push_device, kws_slide_live_push_device, kws_run_classifier_ragged_device; for a live session: the
 * same sequence of pushes on a session of its own at the same slicing or hop.  That holds for scores and raw_scores, for int8 and float32
 * members alike, and `features` is bit-identical to any member's own; through those entry points' contracts the rows match the reference
 * (int8 bit-exact, float32 scores within 1e-6), and the live slide's DIRECT and SHARED paths stay bit-identical to each other.
 * Mode.  These calls always run the exact kernels.  They neither read nor change any member's kws_set_mode state, fast counters
 * (kws_fast_fallback_count / kws_fast_exact_count) or logits tap, and they write no tap.
 * Skipping a member.  scores[k] == NULL skips member k in the scan, the live slide push and the ragged call, which keep nothing per
 * member.  raw_scores == NULL, or a NULL entry of it, means no raw scores for that member (its scores are filtered in place).
 * kws_bank_live_push_device is stricter: a member's moving-average filter must see every window, so a NULL scores[k] is
 * KWS_ERROR_BAD_ARGUMENT and no state changes.  For fewer members make a smaller bank: a handle may be a member of several banks.
 * Empty and refused calls.  Every scores[k] NULL (and features NULL where there is one): KWS_ERROR_BAD_ARGUMENT.  No window, or no clip:
 * EI_IMPULSE_OK, nothing written.  Whatever the single-model entry point refuses is refused with its code before anything is enqueued -- a
 * slicing the stream API refuses, a bad hop or flags, a ragged length outside 1 .. kws_frame_count frames, a stream named twice -- and
 * kws_last_error is set as that entry point sets it.
 * Ordering and locks.  A call or push counts as a call on EVERY member: it takes the members' locks in the bank's fixed order (by address)
 * and brackets every member's scratch, as the bank calls above.  Calls on one bank, its sessions' pushes, resets and counts included, are
 * serialised.
 * Lifetimes.  Destroy sessions before their bank, and banks before their members; a session's destroy waits for its enqueued work.
 * Device memory.  Per live stream ONE carry ring and ONE retained-row ring (kws_live_create's / kws_slide_live_create's) serve all
 * members; the continuous session adds sum_k labels_k x (taps + 1) floats of filter state per stream.  Per-push scratch is the
 * single-model session's, plus the bank's shared feature matrix for one chunk (at most 64 MiB; the ragged call without `features`:
 * B x feature_count floats).  The scan and the ragged call use the FIRST member's scan / ragged scratch with the single-model bounds;
 * no session keeps anything in a member's own scratch between pushes. */
/* kws_scan_recordings_device for K models */
EI_IMPULSE_ERROR kws_bank_scan_recordings_device(kws_bank *b, const int16_t *pcm, const size_t *offsets, const size_t *lengths, size_t R,
                                                 size_t slice_samples, float *const *scores, float *const *raw_scores, void *stream);
/* kws_live_* for K models: one session, one copy of every stream's carry and retained rows, one moving-average state per member */
typedef struct kws_bank_live kws_bank_live;
EI_IMPULSE_ERROR kws_bank_live_create(kws_bank *b, size_t S, size_t slice_samples, kws_bank_live **out);
void kws_bank_live_destroy(kws_bank_live *lv);
EI_IMPULSE_ERROR kws_bank_live_reset(kws_bank_live *lv, const size_t *streams, size_t n);
EI_IMPULSE_ERROR kws_bank_live_window_count(const kws_bank_live *lv, size_t stream, size_t n_new, int finish, size_t *n_windows);
EI_IMPULSE_ERROR kws_bank_live_push_device(kws_bank_live *lv, size_t n, const size_t *streams, const int16_t *pcm, const size_t *offsets,
                                           const size_t *lengths, const int *finish, float *const *scores, float *const *raw_scores,
                                           size_t *n_windows, void *stream);
/* kws_slide_live_* for K models */
typedef struct kws_bank_slide_live kws_bank_slide_live;
EI_IMPULSE_ERROR kws_bank_slide_live_create(kws_bank *b, size_t S, size_t hop_samples, int flags, kws_bank_slide_live **out);
void kws_bank_slide_live_destroy(kws_bank_slide_live *sl);
int kws_bank_slide_live_path(const kws_bank_slide_live *sl);
EI_IMPULSE_ERROR kws_bank_slide_live_reset(kws_bank_slide_live *sl, const size_t *streams, size_t n);
EI_IMPULSE_ERROR kws_bank_slide_live_window_count(const kws_bank_slide_live *sl, size_t stream, size_t n_new, size_t *n_windows);
EI_IMPULSE_ERROR kws_bank_slide_live_push_device(kws_bank_slide_live *sl, size_t n, const size_t *streams, const int16_t *pcm,
                                                 const size_t *offsets, const size_t *lengths, float *const *scores, float *features,
                                                 size_t *n_windows, void *stream);
/* kws_run_classifier_ragged_device for K models: the first member's DSP route once, then every member's network on the full-stride rows */
EI_IMPULSE_ERROR kws_bank_run_classifier_ragged_device(kws_bank *b, const int16_t *pcm, const size_t *offsets, const size_t *lengths, size_t B,
                                                       float *const *scores, float *features, void *stream);

/* ---- routed banks: each clip or stream scored only by the members it names ------------------------------------------------------------
 * A bank call runs every member on every row.  A routed call runs the shared front end once and, for each row, only the members its
 * route names: requests or live streams of many tenants whose models share one DSP block, each scored by its own model and by no other.
 * Route.  A uint32_t per clip, or per stream of a live session: bit k set = member k of the bank, in bank order, scores it.  Routes are
 * HOST data, like `offsets` / `lengths` of the ragged call.  A bit at or above kws_bank_size(b) is KWS_ERROR_BAD_ARGUMENT, kws_last_error
 * names the first offending index and its mask, nothing is enqueued.  A zero mask is legal: the front end still runs for that clip and
 * `features` still gets its row.  routes == NULL means every member: the call then IS the unrouted call (its launches, its bits); so is a
 * call whose routes all name every member.
 * Output.  The layout is the unrouted call's: member k's buffer is [clips or windows of the call][labels_k], rows in the call's order.
 * Only the rows of routed (row, member) pairs are written; every other row of every score buffer -- raw_scores and the moving average's
 * output included -- is left untouched, bit for bit, and the filter state of an unrouted (stream, member) pair is neither read nor
 * written.  `features` holds every row.
 * Parity contract.  A routed (row, member) pair's scores are the bits of the unrouted bank call's and so of that member's own entry point
 * in KWS_MODE_EXACT (int8 bit-exact with the reference, float32 scores within 1e-6); `features` is the unrouted call's, bit for bit.
 * Mode.  Routed calls run the exact launches only, as bank calls do: no mode, fast counter or logits tap is read or written.
 * Launches.  The front end once.  The int8 members of the two-block matrix-core shape share one launch per activation-row width that has a
 * member with a non-empty list (each wave walks its member's list; the grid is sized by the longest list); the other members run their own
 * network launches over their lists; a member nobody names launches nothing.  The K lists are built on the host in one counting pass and
 * uploaded with the call: 4 x (K + routed pairs) bytes of bank-owned device memory, grown on demand (growing synchronises the device).
 * An int8 member outside the matrix-core shape still takes its input tensor from its own batch scratch, grown to the call's rows.
 *   kws_bank_run_classifier_routed_device         kws_bank_run_classifier_batch_device with routes [B]
 *   kws_bank_run_classifier_ragged_routed_device  kws_bank_run_classifier_ragged_device with routes [B]
 *   kws_bank_live_route        sets the routes of n streams (streams, routes: HOST arrays of n entries) of a continuous-mode session.  A
 *                     fresh session routes every stream to every member, and a session that never calls this behaves exactly as
 *                     before.  A member's moving-average filter must see every window of a stream it serves, so a stream's route may
 *                     be set only while the stream is in its start state: after create, kws_bank_live_reset or the push that finished
 *                     it, before anything else was pushed to it; otherwise KWS_ERROR_BAD_ARGUMENT and nothing changes (also for a
 *                     stream index out of range or a bad mask: the first offending entry is named).  kws_bank_live_reset keeps
 *                     routes.  The call waits for the bank's enqueued work.  In kws_bank_live_push_device, scores[k] (and
 *                     raw_scores[k]) may be NULL exactly when no stream named in that push routes to member k; any other NULL is
 *                     KWS_ERROR_BAD_ARGUMENT with no state change.  The moving average stays ONE launch whatever K.
 *   kws_bank_slide_live_route  the same for a live one-shot session; there is no per-member state, so a route may change between any two
 *                     pushes.  kws_bank_slide_live_reset keeps routes.
 * Recording calls and cepstra-in calls.  The three forms below take the unrouted call's arguments plus `routes` (HOST) directly after the
 * count: one route per RECORDING (a window's route is its recording's) or per cepstral matrix.  The contract is the one above:
 *   refusals      a bit at or above kws_bank_size(b): KWS_ERROR_BAD_ARGUMENT, kws_last_error names the first offending recording (or row)
 *                 and its mask; checked before anything is enqueued, nothing is written.  Whatever the unrouted call refuses is refused
 *                 with its code.  R = 0, B = 0 or no window: EI_IMPULSE_OK, nothing written -- after the routes [R] / [B] were checked (a
 *                 bad route of a recording too short for a window is still refused; with R = 0 or B = 0 no route is read).
 *   NULL, all     routes == NULL IS the unrouted call; so is a call in which every recording that has a window (every row) names every
 *                 member: the unrouted launches, no upload.
 *   output        the unrouted call's layout: member k's buffer is [sum_r W_r][labels_k], recording r's windows at rows [wbase_r, wbase_r +
 *                 W_r).  Only the rows of routed (window, member) pairs are written -- in scores, in raw_scores and by the moving average;
 *                 every other row of every score buffer is left untouched, bit for bit.  A scan's filter is fresh per recording, so an
 *                 unrouted (recording, member) pair has no state, and none is read.
 *   features      (slide, cepstra-in) every row, routed or not: the unrouted call's bits.  A recording whose route is 0 still goes through
 *                 the front end, as a zero-mask clip does in the batch call; callers that want to spare that work drop such recordings.
 *   NULL scores   scores[k] == NULL skips member k even where it is routed (the unrouted scan's and slide's rule).  A member no recording
 *                 with windows names, or a member without a buffer, launches nothing.
 *   parity        a routed pair's rows are the bits of the unrouted bank call, so of that member's own kws_scan_recordings_device,
 *                 kws_slide_recordings_device or kws_cmvn_inference_batch_device in KWS_MODE_EXACT (int8 bit-exact with the reference,
 *                 float32 scores within 1e-6); the slide's paths (AUTO, DIRECT, SHARED) stay bit-identical to each other under any routes.
 *   mode          exact launches only; no member's mode, fast counters or logits tap is read or written.
 *   launches      the front end once; per chunk of windows the routed network launches above over that chunk's lists (one upload per chunk:
 *                 4 x (K + routed pairs of the chunk) bytes); the scan's moving average is ONE launch whatever K, over the members some
 *                 recording names, and reads the routes of the recordings that have windows from bank-owned device memory (at most R x 4
 *                 bytes, uploaded with the call).  Ordering, locks and the rest of the device memory: the unrouted forms'.
 * Not routed in this version: the host-buffer and SDK forms. */
EI_IMPULSE_ERROR kws_bank_run_classifier_routed_device(kws_bank *b, const int16_t *pcm, size_t B, const uint32_t *routes,
                                                       float *const *scores, float *features, void *stream);
EI_IMPULSE_ERROR kws_bank_run_classifier_ragged_routed_device(kws_bank *b, const int16_t *pcm, const size_t *offsets, const size_t *lengths,
                                                              size_t B, const uint32_t *routes, float *const *scores, float *features,
                                                              void *stream);
EI_IMPULSE_ERROR kws_bank_scan_recordings_routed_device(kws_bank *b, const int16_t *pcm, const size_t *offsets, const size_t *lengths, size_t R,
                                                        const uint32_t *routes, size_t slice_samples, float *const *scores,
                                                        float *const *raw_scores, void *stream);
EI_IMPULSE_ERROR kws_bank_slide_recordings_routed_device(kws_bank *b, const int16_t *pcm, const size_t *offsets, const size_t *lengths, size_t R,
                                                         const uint32_t *routes, size_t hop_samples, int flags, float *const *scores,
                                                         float *features, void *stream);
EI_IMPULSE_ERROR kws_bank_cmvn_inference_routed_device(kws_bank *b, const float *mfcc, size_t B, const uint32_t *routes, float *const *scores,
                                                       float *features, void *stream);
EI_IMPULSE_ERROR kws_bank_live_route(kws_bank_live *lv, const size_t *streams, size_t n, const uint32_t *routes);
EI_IMPULSE_ERROR kws_bank_slide_live_route(kws_bank_slide_live *sl, const size_t *streams, size_t n, const uint32_t *routes);

/* ---- pools: hundreds of int8 models behind one DSP block, ONE member per row ----------------------------------------------------------
 * A bank serves any subset of at most 16 members of any graph family per row, with one score buffer and one filter state per member.  A
 * pool is its narrow sibling for a service with hundreds of tenants, each with its own keywords trained on the same architecture: up to
 * KWS_POOL_MAX members that share one DSP block, every row (clip or live stream) scored by the ONE member it names, all scores in ONE
 * matrix.  The front end runs once per call, every member's network runs in ONE launch whatever K, and a live session keeps one filter
 * state for all members.
 * Membership.  1 <= K <= KWS_POOL_MAX handles (the range is checked before a member is read), none NULL, none twice, member k equal to
 * member 0 in everything a bank requires (device, DSP block kind and configuration, sampling frequency, raw_sample_count; the bank's rule
 * with the bank's messages): KWS_ERROR_BAD_ARGUMENT otherwise.  Every member must be an int8 graph of the two-block matrix-core shape --
 * two CONV_2D(1-D) + MAX_POOL blocks, FULLY_CONNECTED, SOFTMAX: the stock graph, the shape of both shipped models, the graphs for which
 * kws_nn_kernel_name says "kws_nn_mfma_kernel".  A float32 member, or an int8 member of another family (depthwise, dense stack, strided,
 * 2-D, residual): KWS_ERROR_UNSUPPORTED_MODEL, kws_last_error names the member and the reason.  Label counts may differ:
 * kws_pool_score_stride is the largest.  kws_pool_create changes no member; a member stays usable on its own.
 * Member index.  A uint32_t per clip, or per stream of a live session: the member's index in pool order, or KWS_POOL_NONE.  `member`
 * arrays are HOST data.  An index at or above kws_pool_size(p) that is not KWS_POOL_NONE: KWS_ERROR_BAD_ARGUMENT before anything is
 * enqueued; kws_last_error names the first such row and its value.
 * Output.  scores is [rows][stride] float, device, stride = kws_pool_score_stride(p).  Row i gets, in columns 0 .. labels - 1 of its member,
 * the bits of that member's own KWS_MODE_EXACT call on row i (int8: bit-exact with the reference).  Nothing else of `scores` is written:
 * not the columns at or above the member's label count, not a row that names KWS_POOL_NONE.  `features` ([rows][feature_count], optional)
 * is written for every row, KWS_POOL_NONE rows included, with the bits of the single-model call.
 * Locks and lifetimes.  The pool copies each member's plan record to device memory at creation (1 072 bytes per member, and 4 for its label
 * count); after that it reads only the members' immutable device weights.  A pool call is a call on the pool and on the FIRST member only,
 * whose front end and scratch it uses, for the rules at the top of this file: it holds those two locks and takes no other member's lock or
 * scratch bracket, so calls on the other members run beside it.  Calls on one pool are serialised.  Members outlive the pool; sessions are
 * destroyed before their pool (kws_pool_destroy waits for the pool's enqueued work).
 * Mode.  A pool call always runs the exact kernels, as bank and ragged calls do: no member's mode, fast counter or logits tap is read or
 * written.
 * Launches and memory.  The rows' members become one ascending row list per named member (one counting and one filling pass on the host);
 * the lists are cut into work items of at most kws_pool_item_rows() rows, one workgroup each; items and lists go up in one upload with the
 * call: 16 bytes per item + 4 per named row of pool-owned device memory, grown on demand (growing synchronises the device), like the shared
 * feature matrix of calls without `features`.  A member nobody names costs nothing; rows that all name KWS_POOL_NONE launch no network.
 *   kws_pool_run_classifier_device         run_classifier() for B clips, clip i by member[i].  scores and features both NULL, NULL pool, NULL
 *                     pcm or member with B > 0, B >= 2^31: KWS_ERROR_BAD_ARGUMENT.  B = 0: EI_IMPULSE_OK, nothing written.
 *   kws_pool_run_classifier_ragged_device  the same for clips of their own lengths (kws_run_classifier_ragged_device's contract: the rows
 *                     are the bits of the member's own ragged call); whatever that call refuses is refused with its code.
 *   kws_pool_live_*   kws_live_* for a pool: one session of S streams, one copy of every stream's carried samples and retained rows, filter
 *                     state [S][stride][taps + 1] floats in total.  Each stream is assigned to one member or to none; a fresh session assigns
 *                     every stream to KWS_POOL_NONE.  kws_pool_live_assign(lv, streams, n, member) sets the members of n streams (HOST
 *                     arrays).  A stream's moving-average filter must see every window through one member, so a stream may be assigned only
 *                     in its start state: after create, kws_pool_live_reset or the push that finished it, before anything else was pushed
 *                     to it; otherwise -- or for a stream out of range or named twice, or a bad index -- KWS_ERROR_BAD_ARGUMENT, the first
 *                     offending entry is named, nothing changes.  Reset keeps assignments.  The call waits for the pool's enqueued work.
 *                     kws_pool_live_push_device has kws_live_push_device's arguments; scores and raw_scores (optional) are
 *                     [windows of the push][stride], entry after entry.  An assigned stream's rows, filtered and raw, are the bits of its
 *                     member's own kws_live_* session fed the same pushes.  A push to an unassigned stream advances its carry and counts
 *                     its windows in n_windows, but writes no row and touches no filter state.  The moving average is ONE launch per push.
 * Recordings, live one-shot windows, cepstra in.  What a bank serves of these a pool serves too, each being the first member's pipeline
 * with the pool's finishing step.  scores (and raw_scores) are [windows of the call][stride] in the order of the single-model call; a
 * window's member is its recording's (scan, slide) or its stream's (live).  A window of a recording or stream that names KWS_POOL_NONE
 * keeps its place in the matrix.  A named window's row holds, in columns 0 .. labels - 1 of its member, the bits of that member's own
 * KWS_MODE_EXACT call on that recording alone (live: of the member's own session fed the same pushes), raw and filtered alike.  Nothing
 * else of scores / raw_scores is written: not the columns at or above the member's label count, not a KWS_POOL_NONE window's row, not a row
 * past the call.  `features`, where a call has it, is written for every window or row, KWS_POOL_NONE ones included, with the single-model
 * call's bits.  The front end runs ONCE through the first member for ALL recordings or streams of the call, the ones that name nobody
 * included -- its launches are exactly those of the first member's own call -- so a caller who wants no work done for a recording drops it
 * from the call.  The networks are one launch per gathered chunk of windows (64 MiB of cepstra) whatever K.  Every refusal comes before
 * anything is enqueued and names the first offending entry: an index at or above K that is not KWS_POOL_NONE (named as "recording", "row"
 * or "entry"), no output requested, a NULL pool or session, NULL member with a non-empty call, a stream out of range or named twice
 * (KWS_ERROR_BAD_ARGUMENT), and whatever the single-model call refuses, with its code (a bad slicing, hop or flags, too many windows, NULL
 * lengths).  Locks: the pool's and the first member's, as above.
 *   kws_pool_scan_recordings_device   kws_scan_recordings_device for a pool, recording r by member[r].  scores is required; with raw_scores
 *                     == NULL the moving average filters in place.  A fresh filter per recording; the moving average is ONE launch per call,
 *                     and none when no recording with windows names a member.  The members of the recordings that have windows go up with
 *                     the call (4 bytes each).
 *   kws_pool_slide_recordings_device  kws_slide_recordings_device for a pool, recording r by member[r].  scores and features both NULL:
 *                     refused.  The bound on windows x labels holds at the stride (kws_slide_plan of the member with the most labels).
 *   kws_pool_cmvn_inference_device    kws_cmvn_inference_batch_device for a pool: B rows of cepstra, row i by member[i].
 *   kws_pool_slide_live_*   kws_slide_live_* for a pool: one session of S streams on the first member; no state per member.  A fresh
 *                     session assigns every stream to KWS_POOL_NONE; kws_pool_slide_live_assign sets the members of n streams (HOST arrays;
 *                     host-only: no device table and no wait) and may change a stream's member between any two pushes, as
 *                     kws_bank_slide_live_route may.  Reset keeps assignments.  kws_pool_slide_live_push_device has
 *                     kws_slide_live_push_device's arguments; scores is [windows of the push][stride], entry after entry.  A push to an
 *                     unassigned stream advances its carry and counts its windows in n_windows, but writes no score row.
 * Not built: float32 and other-family members, device-resident member arrays, KWS_MODE_FAST, a tenant object lighter than a kws_handle. */
#define KWS_POOL_MAX 4096
#define KWS_POOL_NONE 0xffffffffu
typedef struct kws_pool kws_pool;
typedef struct kws_pool_live kws_pool_live;
typedef struct kws_pool_slide_live kws_pool_slide_live;
EI_IMPULSE_ERROR kws_pool_create(kws_handle *const *members, size_t K, kws_pool **out);
void kws_pool_destroy(kws_pool *p);
size_t kws_pool_size(const kws_pool *p);
kws_handle *kws_pool_member(const kws_pool *p, size_t k);                  /* NULL for k >= K */
size_t kws_pool_score_stride(const kws_pool *p);                           /* the most labels any member has */
int kws_pool_item_rows(void);                                              /* rows of one work item at most (diagnostics; tests place lists at its edges) */
EI_IMPULSE_ERROR kws_pool_run_classifier_device(kws_pool *p, const int16_t *pcm, size_t B, const uint32_t *member, float *scores,
                                                float *features, void *stream);
EI_IMPULSE_ERROR kws_pool_run_classifier_ragged_device(kws_pool *p, const int16_t *pcm, const size_t *offsets, const size_t *lengths, size_t B,
                                                       const uint32_t *member, float *scores, float *features, void *stream);
EI_IMPULSE_ERROR kws_pool_live_create(kws_pool *p, size_t S, size_t slice_samples, kws_pool_live **out);
void kws_pool_live_destroy(kws_pool_live *lv);
EI_IMPULSE_ERROR kws_pool_live_reset(kws_pool_live *lv, const size_t *streams, size_t n);
EI_IMPULSE_ERROR kws_pool_live_assign(kws_pool_live *lv, const size_t *streams, size_t n, const uint32_t *member);
EI_IMPULSE_ERROR kws_pool_live_window_count(const kws_pool_live *lv, size_t stream, size_t n_new, int finish, size_t *n_windows);
EI_IMPULSE_ERROR kws_pool_live_push_device(kws_pool_live *lv, size_t n, const size_t *streams, const int16_t *pcm, const size_t *offsets,
                                           const size_t *lengths, const int *finish, float *scores, float *raw_scores, size_t *n_windows,
                                           void *stream);
EI_IMPULSE_ERROR kws_pool_scan_recordings_device(kws_pool *p, const int16_t *pcm, const size_t *offsets, const size_t *lengths, size_t R,
                                                 const uint32_t *member /* [R] */, size_t slice_samples, float *scores, float *raw_scores, void *stream);
EI_IMPULSE_ERROR kws_pool_slide_recordings_device(kws_pool *p, const int16_t *pcm, const size_t *offsets, const size_t *lengths, size_t R,
                                                  const uint32_t *member /* [R] */, size_t hop_samples, int flags, float *scores, float *features,
                                                  void *stream);
EI_IMPULSE_ERROR kws_pool_cmvn_inference_device(kws_pool *p, const float *mfcc, size_t B, const uint32_t *member /* [B] */, float *scores,
                                                float *features, void *stream);
EI_IMPULSE_ERROR kws_pool_slide_live_create(kws_pool *p, size_t S, size_t hop_samples, int flags, kws_pool_slide_live **out);
void kws_pool_slide_live_destroy(kws_pool_slide_live *sl);
int kws_pool_slide_live_path(const kws_pool_slide_live *sl);
EI_IMPULSE_ERROR kws_pool_slide_live_reset(kws_pool_slide_live *sl, const size_t *streams, size_t n);
EI_IMPULSE_ERROR kws_pool_slide_live_assign(kws_pool_slide_live *sl, const size_t *streams, size_t n, const uint32_t *member);
EI_IMPULSE_ERROR kws_pool_slide_live_window_count(const kws_pool_slide_live *sl, size_t stream, size_t n_new, size_t *n_windows);
EI_IMPULSE_ERROR kws_pool_slide_live_push_device(kws_pool_slide_live *sl, size_t n, const size_t *streams, const int16_t *pcm,
                                                 const size_t *offsets, const size_t *lengths, float *scores, float *features, size_t *n_windows,
                                                 void *stream);

/* ---- multi-GPU: clips shard contiguously over the GPUs of one node (rank r owns clips [r*B, (r+1)*B)), tables are
 * replicated, nothing is exchanged inside the pipeline; the one collective is the all-gather of the per-clip scores over xGMI.
 * It goes through RCCL's C API (librccl is opened on first use: single-GPU applications do not need it).  One process per GPU:
 * rank 0 obtains the 128-byte id and hands it to the other ranks with whatever started them (environment, file, MPI, a socket --
 * bench.py uses torch.distributed); every rank then creates its communicator on its own device.
 *   all_scores [world_size * clips_per_rank][label_count] float, device: rank-major = global clip order.  Asynchronous on
 * `stream` (the same stream as the batch call that produced local_scores: no synchronisation in between). */
#define KWS_COMM_ID_BYTES 128
typedef struct kws_comm kws_comm;
EI_IMPULSE_ERROR kws_comm_unique_id(void *id, size_t nbytes);
EI_IMPULSE_ERROR kws_comm_create(const void *id, size_t nbytes, int world_size, int rank, int device, kws_comm **out);
int kws_comm_world_size(const kws_comm *c);
int kws_comm_rank(const kws_comm *c);
int kws_comm_ranks_seen(const kws_comm *c);     /* ncclCommCount of the communicator: what RCCL itself says (kws_comm_create refuses a mismatch) */
int kws_comm_rccl_version(void);                /* ncclGetVersion of the loaded librccl (0: not loadable); its major version must be the rccl.h's this library was built with */
/* Waits until everything enqueued on `stream` (the batch call and its all-gather) has completed -- against a deadline (environment variable
 * KWS_COMM_TIMEOUT_MS, default 120 000; kws_comm_create's wait for the other ranks uses the same one): if a peer has failed or nothing moves,
 * the communicator is aborted (ncclCommAbort) and KWS_ERROR_HIP returned instead of hanging. */
EI_IMPULSE_ERROR kws_comm_wait(kws_comm *c, void *stream);
EI_IMPULSE_ERROR kws_allgather_scores(kws_comm *c, const float *local_scores, float *all_scores, size_t clips_per_rank, int label_count,
                                      void *stream);
void kws_comm_destroy(kws_comm *c);

/* ---- the step before the path: mix_audio of /root/reference/dataset-curation.py:93-137, batched on the GPU, so that a
 * harness can feed real keyword / background recordings instead of synthetic clips.  Inputs are float32 waveforms already at the
 * model's sampling rate (what librosa.load(sr = 16000, mono = True) returns: resampling is NOT part of this call):
 *   words [n_clips] waveforms of word_len[b] samples at words + b * word_stride (device; NULL = background noise only),
 *   noise one background track (device; NULL = no background), start[b] = first sample of clip b's window in it (the reference
 *   draws it with random.randint(0, len(noise) - n); the caller supplies it),
 *   out [n_clips][n] int16 = PCM16(0.5 * word_vol * word + 0.5 * bg_vol * noise[start .. start + n)), words padded with zeros or
 *   truncated to n samples.  PARITY UNPINNED (librosa / soundfile unavailable when this was written): held to the restatement in
 *   oracle/ only. */
EI_IMPULSE_ERROR kws_mix_audio_device(const float *words, const int *word_len, size_t word_stride, const float *noise, size_t noise_len,
                                      const int *start, float word_vol, float bg_vol, size_t n_clips, size_t n, int16_t *out, void *stream);

/* ---- the rest of that step: what librosa.load(path, sr = 16000, mono = True) (dataset-curation.py:111,126) does with a WAV file before
 * mix_audio sees it -- decode, mix down to mono, resample.  PARITY UNPINNED like kws_mix_audio_device (no librosa / soundfile / resampy in
 * reach): the decoder follows libsndfile's published conversion rules (integer PCM / 2^(bits - 1); 8-bit WAV is unsigned), the mono mix-down
 * NumPy's mean over the channels, the resampler the published design of resampy's "kaiser_best" filter (Kaiser-windowed sinc, 64 zero
 * crossings); tests hold them to Python's `wave` / scipy.io.wavfile and to scipy.signal.resample_poly within a stated tolerance.
 *   kws_wav_info_from_memory  container facts of a RIFF/WAVE image in memory (PCM 8 / 16 / 24 / 32 bit, IEEE float 32, also as
 *                             WAVE_FORMAT_EXTENSIBLE; unknown chunks are skipped)
 *   kws_wav_decode_mono       host: samples -> float32 in [-1, 1), channels averaged; out == NULL only reports *frames / *sample_rate
 *   kws_resample_length       ceil(n_in * sr_out / sr_in), librosa's output length
 *   kws_resample_device       device -> device; sr_in == sr_out copies (librosa.load leaves such a file alone).  The reference's behaviour:
 *                             resampy's published loop (a wing walks the table in truncated integer steps with one interpolation factor,
 *                             float32 accumulation, floor(n ratio) samples, then librosa's fix_length zero padding up to ceil(n ratio))
 *   kws_resample_device_ex    flags = KWS_RESAMPLE_EXACT_POSITIONS: every tap's table position exact, products summed in double, every
 *                             sample computed -- 5e-8 .. 7e-7 from the analytic signal where the reference's stepping is 6e-4 .. 2e-3 away */
#define KWS_RESAMPLE_EXACT_POSITIONS 1
typedef struct {
    int channels, sample_rate, bits_per_sample, is_float;
    size_t frames, data_offset;
} kws_wav_info;
EI_IMPULSE_ERROR kws_wav_info_from_memory(const void *bytes, size_t nbytes, kws_wav_info *info);
EI_IMPULSE_ERROR kws_wav_decode_mono(const void *bytes, size_t nbytes, float *out, size_t out_cap, size_t *frames, int *sample_rate);
size_t kws_resample_length(size_t n_in, int sr_in, int sr_out);
EI_IMPULSE_ERROR kws_resample_device(const float *in, size_t n_in, int sr_in, float *out, size_t n_out, int sr_out, void *stream);
EI_IMPULSE_ERROR kws_resample_device_ex(const float *in, size_t n_in, int sr_in, float *out, size_t n_out, int sr_out, int flags, void *stream);

/* deterministic synthetic clips generated directly in HBM (include/kws/kws_synth.h) */
EI_IMPULSE_ERROR kws_synth_clips_device(uint32_t seed, uint32_t first_clip, uint32_t n_clips, uint32_t clip_len,
                                        int16_t *out, void *stream);

/* device memory helpers so that a pure-C caller needs no HIP headers */
EI_IMPULSE_ERROR kws_device_malloc(void **ptr, size_t nbytes);
EI_IMPULSE_ERROR kws_device_free(void *ptr);
EI_IMPULSE_ERROR kws_memcpy_h2d(void *dst, const void *src, size_t nbytes);
EI_IMPULSE_ERROR kws_memcpy_d2h(void *dst, const void *src, size_t nbytes);
EI_IMPULSE_ERROR kws_device_synchronize(void);

#ifdef __cplusplus
}
#endif
#endif
