// kws_bank.h -- what the bank's units share (internal to libkws_mi355x.so): kws_bank.cpp and kws_bank_kernels.hip, and the bank forms of the
// window pipelines, kws_bank_windows.cpp and kws_bank_windows_kernels.hip.
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

// One moving-average launch for every member of a continuous-mode bank call (kws_bank_windows_kernels.hip): member slot i filters
// raw[i] [windows][labels[i]] into scores[i] (may be the same buffer); a live push keeps member i's filters at maf + base[i], stream after
// stream, [S][labels[i]][taps + 1].  By value in the launch arguments, as KwsBankOut.
struct KwsBankMaf {
    int n;
    int labels[KWS_BANK_MAX];
    const float *raw[KWS_BANK_MAX];
    float *scores[KWS_BANK_MAX];
    long long base[KWS_BANK_MAX];
};
int kws_launch_bank_maf_scan(const KwsBankMaf &M, const long long *wbase, int n_rec, hipStream_t stream);
int kws_launch_bank_maf_live(const KwsBankMaf &M, const long long *meta, int n_act, int k_full, float *maf, hipStream_t stream);

// ---- host side (kws_bank.cpp, kws_bank_windows.cpp: the units that include kws_internal.h first) ---------------------------------------------
#ifdef KWS_INTERNAL
#include <memory>

struct kws_bank {
    std::vector<kws_handle *> m;           // members, in the caller's order
    std::vector<kws_handle *> by_addr;     // the same, in the order their locks are taken
    int device = 0;
    KwsBankRec *d_rec = nullptr;           // [K] (int8 members' entries are filled)
    float *feat = nullptr;                 // the shared feature matrix of calls without `features`
    size_t feat_cap = 0;
    hipEvent_t ev = nullptr;               // end of the last call's work
    bool ev_used = false;
    std::mutex mu;
};

// every member's lock in one order whatever the order of the members (two banks over the same handles cannot deadlock), and every
// member's scratch bracket: the call is a call on each of them (kws.h: streams and concurrency)
struct BankUse {
    std::unique_lock<std::mutex> own;
    std::vector<std::unique_lock<std::mutex>> locks;
    std::vector<std::unique_ptr<ScratchUse>> uses;        // released before the locks (declared after them)
    kws_bank *b;
    hipStream_t s;
    // skip_first: the pipeline runners bracket the first member themselves (kws_slide_run and the runners of kws_internal.h)
    BankUse(kws_bank *b_, hipStream_t s_, bool skip_first) : own(b_->mu), b(b_), s(s_)
    {
        for (kws_handle *h : b->by_addr) locks.emplace_back(h->mu);
        for (size_t k = skip_first ? 1 : 0; k < b->m.size(); ++k) uses.emplace_back(new ScratchUse(b->m[k], s));
    }
    ~BankUse()
    {
        if (b->ev && hipEventRecord(b->ev, s) == hipSuccess) b->ev_used = true;
    }
};

// kws_bank.cpp.  bank_networks: every member's network from the feature matrix feat [B][F] (device); scores[k] + row0 * labels of member k
// is where its rows go.  bank_window_finish: the finishing step of a chunk of gathered windows for a bank (a kws_slide_finish_fn over a
// BankWindows): cmvnw (the MFE normalisation) once through the first member, then every member.
KWS_INTERNAL EI_IMPULSE_ERROR bank_networks(kws_bank *b, const float *feat, size_t B, float *const *scores, size_t row0, hipStream_t s);
KWS_INTERNAL bool bank_wants_nothing(const kws_bank *b, float *const *scores, const float *features);
struct BankWindows {
    kws_bank *b;
    float *const *scores;          // [K]: where member k's rows go (NULL: skipped)
    float *features;               // the caller's [windows][F], or NULL: the bank's shared matrix, a chunk at a time
};
KWS_INTERNAL EI_IMPULSE_ERROR bank_window_finish(void *ctx, float *win, size_t n, size_t g0, hipStream_t s);
#endif
