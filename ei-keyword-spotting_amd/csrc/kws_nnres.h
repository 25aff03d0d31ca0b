// kws_nnres.h -- the residual trunks: what kws_nnres_int8.hip / kws_nnres_f32.hip share with the plan builder (kws_plan.cpp) and with the
// launchers of the dense stacks (kws_nn_int8.hip launch_dense_i8, kws_nn_f32.hip launch_dense_f32), which call them chunk by chunk of the hand-off buffer.
#pragma once
#include <hip/hip_runtime.h>
#include "kws_plan.h"

// waves per workgroup: the most that fit the LDS budget, from 16 down to 2 (the 2-D trunks' budgets); the waves of a workgroup share one copy of the
// weights, requantisation constants and ADD tables.  Below KWS_NNRES_WAVES_STAGE (the floor of DESIGN 4.17) only what would be refused otherwise runs: a
// float inverted residual's expanded image; the float plan stages filters in LDS only while the graph still fits at KWS_NNRES_WAVES_STAGE.
#define KWS_NNRES_WAVES_MIN 2
#define KWS_NNRES_WAVES_STAGE 4
#define KWS_NNRES_WAVES_MAX 16
#define KWS_NNRES_LDS_I8 (158 * 1024)
#define KWS_NNRES_LDS_F32 (150 * 1024)
#define KWS_NNRES_ADD_TAB_BYTES 2048       // int8 ADD: two tables of 256 int32

// LDS bytes at n_waves waves per workgroup, and the wave count the launcher picks (0: the graph does not fit at KWS_NNRES_WAVES_MIN -- refused at
// kws_create); kws_plan.cpp
size_t kws_nnres_smem_bytes(const KwsResPlan &N, int n_waves);
int kws_nnres_waves(const KwsResPlan &N);
size_t kws_nnres_f32_smem_bytes(const KwsResPlanF32 &N, int n_waves);
int kws_nnres_f32_waves(const KwsResPlanF32 &N);

// The trunk over list entries ci0 .. ci1 - 1 (sel: kws_device.h's clip list, or NULL): every step, the last one's output -- flattened NHWC, the bytes /
// floats of the reference's tensor -- to handoff [ci - ci0][out_n].  int8: tap_pooled (or NULL) receives every step's (pooled) output per clip, one after
// another, rows of pooled_stride bytes.  Returns 0 or a hipError_t.
// Weak references, as kws_nn2d.h's: a link without the trunks' translation units leaves them NULL, and the dense launchers answer
// hipErrorInvalidDeviceFunction: a missing kernel is an error, never a fall-back.
__attribute__((weak)) int kws_launch_nnres_trunk(const KwsResPlan &N, const int8_t *q_in, int n_clips, int8_t *handoff, int ci0, int ci1, int8_t *tap_pooled, int pooled_stride,
                           const int *sel, int n_cu, hipStream_t stream);
__attribute__((weak)) int kws_launch_nnres_f32_trunk(const KwsResPlanF32 &N, const float *features, int n_clips, float *handoff, int ci0, int ci1, const int *sel, int n_cu,
                               hipStream_t stream);
