// kws_bank.h -- what kws_bank.cpp and kws_bank_kernels.hip share (internal to libkws_mi355x.so).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kws_plan.h"

#define KWS_BANK_MAX 16            // members of a bank (include/kws/kws.h)

// One record per member, in HBM for the bank's lifetime (written once by kws_bank_create): what the bank kernels need of an int8 member.
struct KwsBankRec {
    KwsNnPlan N;
    float in_scale;                // input tensor quantisation (N's own, next to the plan for the quantise-on-load)
    int in_zp;
};

// What changes from call to call travels in the launch arguments, so that no call writes the records: the members one launch serves
// (slot = blockIdx.y) and where their scores go.
struct KwsBankOut {
    int n;
    int rec[KWS_BANK_MAX];         // slot -> record
    float *scores[KWS_BANK_MAX];   // slot -> [n_clips][fc_out]
};

struct KwsBankQuant {
    int n;
    int zp[KWS_BANK_MAX];
    float scale[KWS_BANK_MAX];
    int8_t *q[KWS_BANK_MAX];       // [n] each
};

int kws_launch_bank_nn_mfma(const KwsBankRec *recs, const KwsBankOut &out, int cp, const float *features, int n_clips, int grid_cap, hipStream_t stream);
int kws_launch_bank_quantize(const float *features, size_t n, const KwsBankQuant &Q, hipStream_t stream);
