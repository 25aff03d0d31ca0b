// kws_ragged.h -- ragged batches (kws_run_classifier_ragged_device; internal to libkws_mi355x.so): the per-clip descriptor the ragged form of
// kws_mfcc8_kernel reads, and the launchers of kws_ragged_kernels.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kws_plan.h"

// One clip of a ragged batch: where its samples are, how many, and the frames that fit.  16 bytes: one scalar load per clip.
struct KwsRaggedClip {
    const int16_t *x;    // first sample.  The kernel's table: 16-byte aligned (the clip in place, or its slot of the staging buffer);
                         // a staging / gather list: the clip where the caller put it, any alignment
    int length;          // samples; x[length - 1] is the wrap sample
    int frames;          // the kernel's table: 1 .. the model's frame count; the grouped route's list: the clip's row of the outputs
};
// what the ragged form takes from tables instead of the plan
struct KwsRaggedArgs {
    const KwsRaggedClip *clips;   // [n_clips]
    const int *pad_maps;          // [frames + 1][map_stride]: row nfr is numpy::pad_1d_symmetric's row map for nfr rows
    int map_stride;
};

// extract_mfcc_features (+ quantisation) of n_clips clips of their own lengths in ONE launch: rows of out_stride values, zero-filled behind
// the frames that fit.  hipErrorInvalidValue: no instantiation for this plan (the caller routes such plans to the grouped route).
int kws_launch_mfcc_ragged(const KwsDspPlan &P, const KwsRaggedArgs &R, int n_clips, float *features, int8_t *q_out, float in_scale, int in_zp,
                           int out_stride, int grid_cap, hipStream_t stream);
bool kws_mfcc_ragged_serves(const KwsDspPlan &P);
// list[j] -> slot j of dst (slot_stride samples apart, the samples behind a clip's own zeroed); wrap (optional): x[length - 1] / 32768 per slot
int kws_launch_ragged_stage(const KwsRaggedClip *list, int n, int16_t *dst, int slot_stride, float *wrap, hipStream_t stream);
// packed [n][n_valid] -> rows list[j].frames of features / q_out ([.][row_len]), +0.0f / quantise(0) behind the n_valid values
int kws_launch_ragged_scatter(const float *packed, const KwsRaggedClip *list, int n, int n_valid, int row_len, float *features, int8_t *q_out,
                              float in_scale, int in_zp, hipStream_t stream);
