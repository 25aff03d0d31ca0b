// kws_bank_windows.cpp -- the bank forms of the window pipelines (contract in include/kws/kws.h): recording scans and live streams in
// continuous mode, live one-shot windows and clips of their own lengths for K models that share one DSP block.
//   kws_bank_scan_recordings_device         kws_scan_run      (kws_scan.cpp)
//   kws_bank_live_*                         kws_live_run      (kws_live.cpp), on a session of the first member opened without filter state
//   kws_bank_slide_live_*                   kws_slide_live_run (kws_slide_live.cpp), on a session of the first member
//   kws_bank_run_classifier_ragged_device   kws_ragged_run    (kws_ragged.cpp) with the network skipped
// Each is the first member's pipeline runner (kws_internal.h) with the bank's hooks, as kws_bank_slide_recordings_device is kws_slide_run with
// bank_window_finish: staging, the spectral kernels, gathering, carry and retained rows are the first member's and run ONCE; every chunk of
// gathered windows ends in bank_window_finish (cmvnw once, then every member's network: kws_bank.cpp), and continuous mode's moving average
// is ONE launch of kws_bank_maf_kernel for all members (kws_bank_windows_kernels.hip).  What is per member: its scores, its raw scores and,
// in a live session, its filters -- sum_k labels_k x (taps + 1) floats per stream, in one allocation of the session.
// These are the launches of KWS_MODE_EXACT: nothing here reads or writes a member's mode, fast counters or logits tap, and no hook of the
// bank's asks for the idle finishing call (finish_idle) that the single-model pushes use to reset their counters.
#include "kws_internal.h"
#include "kws_bank.h"

#include "../../include/kws/ei_compat.h"

#include <algorithm>

static const int kBankTaps = EI_CLASSIFIER_SLICES_PER_MODEL_WINDOW >> 1;

static size_t bank_max_labels(const kws_bank *b)
{
    size_t c = 0;
    for (const kws_handle *h : b->m) c = std::max(c, h->model.labels.size());
    return c;
}

// Continuous mode for a bank: the chunks' raw scores go where each member's moving average reads them -- its raw_scores, or its scores
// (filtered in place) -- and the filter step is one launch over the members that are not skipped.
struct BankContinuous {
    BankWindows w;                         // (first: bank_window_finish reads it)
    float *raw[KWS_BANK_MAX];              // w.scores points here
    float *const *scores;
    int k_full;                            // the live form (maf != NULL): the layout's first window step
    float *maf;
    const long long *base;                 // [K] floats before member k's filters
    BankContinuous(kws_bank *b, float *const *scores_, float *const *raw_scores, int k_full_ = 0, float *maf_ = nullptr, const long long *base_ = nullptr)
        : w{ b, raw, nullptr }, scores(scores_), k_full(k_full_), maf(maf_), base(base_)
    {
        for (size_t k = 0; k < b->m.size(); ++k) raw[k] = !scores[k] ? nullptr : raw_scores && raw_scores[k] ? raw_scores[k] : scores[k];
    }
    BankContinuous(const BankContinuous &) = delete;       // (w.scores points into this object)
};
static EI_IMPULSE_ERROR bank_continuous_maf(void *ctx, const long long *meta, int n, hipStream_t s)
{
    BankContinuous &c = *(BankContinuous *)ctx;
    kws_bank *b = c.w.b;
    KwsBankMaf M{};
    for (size_t k = 0; k < b->m.size(); ++k) {
        if (!c.scores[k]) continue;
        M.labels[M.n] = (int)b->m[k]->model.labels.size();
        M.raw[M.n] = c.raw[k];
        M.scores[M.n] = c.scores[k];
        M.base[M.n] = c.base ? c.base[k] : 0;
        ++M.n;
    }
    KWS_LAUNCH_TRY("bank moving-average kernel", c.maf ? kws_launch_bank_maf_live(M, meta, n, c.k_full, c.maf, s) : kws_launch_bank_maf_scan(M, meta, n, s));
    return EI_IMPULSE_OK;
}

// the ragged call's finishing step: the DSP route has written the full-stride feature rows; every member's network reads them
static EI_IMPULSE_ERROR bank_ragged_finish(void *ctx, float *f, size_t B, size_t, hipStream_t s)
{
    BankWindows &c = *(BankWindows *)ctx;
    return bank_networks(c.b, f, B, c.scores, 0, s);
}

// (the sessions: the bank, the first member's session -- carry, retained rows, mirrors, per-push scratch: ONE copy -- and what is per member)
struct kws_bank_live {
    kws_bank *b = nullptr;
    kws_live *core = nullptr;
    ScanLayout L;
    float *maf = nullptr;                  // state in HBM: member k's [S][labels_k][taps + 1] at base[k]
    std::vector<long long> base;
};
struct kws_bank_slide_live {
    kws_bank *b = nullptr;
    kws_slide_live *core = nullptr;
};

// the end of the bank's latest call, this session's last push included (BankUse records it), before a session's memory goes
static void bank_wait(kws_bank *b)
{
    (void)hipSetDevice(b->device);
    if (b->ev && b->ev_used) (void)hipEventSynchronize(b->ev);
}

extern "C" {
#pragma GCC visibility push(default)

EI_IMPULSE_ERROR kws_bank_scan_recordings_device(kws_bank *b, const int16_t *pcm, const size_t *offsets, const size_t *lengths, size_t R,
                                                 size_t slice_samples, float *const *scores, float *const *raw_scores, void *stream)
{
    if (!b || !scores) return fail(KWS_ERROR_BAD_ARGUMENT, "null argument");
    if (bank_wants_nothing(b, scores, nullptr)) return fail(KWS_ERROR_BAD_ARGUMENT, "no output requested: every scores[k] is NULL");
    HIP_TRY(hipSetDevice(b->device));
    hipStream_t s = (hipStream_t)stream;
    BankUse use(b, s, true);
    BankContinuous ctx(b, scores, raw_scores);
    return kws_scan_run(b->m[0], pcm, offsets, lengths, R, slice_samples, bank_max_labels(b), 0, bank_window_finish, bank_continuous_maf, &ctx, s);
}

EI_IMPULSE_ERROR kws_bank_live_create(kws_bank *b, size_t S, size_t slice_samples, kws_bank_live **out)
{
    if (out) *out = nullptr;
    if (!b || !out) return fail(KWS_ERROR_BAD_ARGUMENT, "bad argument");
    std::unique_ptr<kws_bank_live> lv(new kws_bank_live());
    lv->b = b;
    EI_IMPULSE_ERROR e = kws_live_open(b->m[0], S, slice_samples, 0, &lv->core);
    if (e) return e;
    (void)scan_layout(b->m[0], slice_samples, &lv->L);             // (kws_live_open has accepted the slicing)
    long long floats = 0;
    for (const kws_handle *h : b->m) {
        lv->base.push_back(floats);
        floats += (long long)(S * h->model.labels.size() * (kBankTaps + 1));
    }
    // (a stream's filters are read only once it has had a window; cleared so that no stale value can ever reach a result)
    if (hipMalloc((void **)&lv->maf, (size_t)floats * sizeof(float)) != hipSuccess || hipMemset(lv->maf, 0, (size_t)floats * sizeof(float)) != hipSuccess) {
        if (lv->maf) (void)hipFree(lv->maf);
        kws_live_destroy(lv->core);
        return fail(KWS_ERROR_HIP, "bank live session allocation failed");
    }
    *out = lv.release();
    return EI_IMPULSE_OK;
}

void kws_bank_live_destroy(kws_bank_live *lv)
{
    if (!lv) return;
    {
        std::lock_guard<std::mutex> lk(lv->b->mu);
        bank_wait(lv->b);
        kws_live_destroy(lv->core);
        if (lv->maf) (void)hipFree(lv->maf);
    }
    delete lv;
}

EI_IMPULSE_ERROR kws_bank_live_reset(kws_bank_live *lv, const size_t *streams, size_t n)
{
    if (!lv) return fail(KWS_ERROR_BAD_ARGUMENT, "null argument");
    std::lock_guard<std::mutex> lk(lv->b->mu);
    return kws_live_reset(lv->core, streams, n);
}

EI_IMPULSE_ERROR kws_bank_live_window_count(const kws_bank_live *lv, size_t stream, size_t n_new, int finish, size_t *n_windows)
{
    if (!lv) return fail(KWS_ERROR_BAD_ARGUMENT, "null argument");
    std::lock_guard<std::mutex> lk(lv->b->mu);
    return kws_live_window_count(lv->core, stream, n_new, finish, n_windows);
}

EI_IMPULSE_ERROR kws_bank_live_push_device(kws_bank_live *lv, size_t n, const size_t *streams, const int16_t *pcm, const size_t *offsets,
                                           const size_t *lengths, const int *finish, float *const *scores, float *const *raw_scores,
                                           size_t *n_windows, void *stream)
{
    if (!lv) return fail(KWS_ERROR_BAD_ARGUMENT, "null argument");
    kws_bank *b = lv->b;
    // every member's filter must see every window: no member is skipped in a push
    for (size_t k = 0; scores && k < b->m.size(); ++k)
        if (!scores[k]) return fail(KWS_ERROR_BAD_ARGUMENT, "scores[%zu] is NULL: a live push skips no member", k);
    HIP_TRY(hipSetDevice(b->device));
    hipStream_t s = (hipStream_t)stream;
    BankUse use(b, s, true);
    float *const none[KWS_BANK_MAX] = { nullptr };
    BankContinuous ctx(b, scores ? scores : none, raw_scores, (int)lv->L.k_full, lv->maf, lv->base.data());
    return kws_live_run(lv->core, n, streams, pcm, offsets, lengths, finish, scores, n_windows, bank_max_labels(b), 0, 0, bank_window_finish,
                        bank_continuous_maf, &ctx, s);
}

EI_IMPULSE_ERROR kws_bank_slide_live_create(kws_bank *b, size_t S, size_t hop_samples, int flags, kws_bank_slide_live **out)
{
    if (out) *out = nullptr;
    if (!b || !out) return fail(KWS_ERROR_BAD_ARGUMENT, "bad argument");
    std::unique_ptr<kws_bank_slide_live> sl(new kws_bank_slide_live());
    sl->b = b;
    EI_IMPULSE_ERROR e = kws_slide_live_create(b->m[0], S, hop_samples, flags, &sl->core);
    if (e) return e;
    *out = sl.release();
    return EI_IMPULSE_OK;
}

void kws_bank_slide_live_destroy(kws_bank_slide_live *sl)
{
    if (!sl) return;
    {
        std::lock_guard<std::mutex> lk(sl->b->mu);
        bank_wait(sl->b);
        kws_slide_live_destroy(sl->core);
    }
    delete sl;
}

int kws_bank_slide_live_path(const kws_bank_slide_live *sl) { return sl ? kws_slide_live_path(sl->core) : 0; }

EI_IMPULSE_ERROR kws_bank_slide_live_reset(kws_bank_slide_live *sl, const size_t *streams, size_t n)
{
    if (!sl) return fail(KWS_ERROR_BAD_ARGUMENT, "null argument");
    std::lock_guard<std::mutex> lk(sl->b->mu);
    return kws_slide_live_reset(sl->core, streams, n);
}

EI_IMPULSE_ERROR kws_bank_slide_live_window_count(const kws_bank_slide_live *sl, size_t stream, size_t n_new, size_t *n_windows)
{
    if (!sl) return fail(KWS_ERROR_BAD_ARGUMENT, "null argument");
    std::lock_guard<std::mutex> lk(sl->b->mu);
    return kws_slide_live_window_count(sl->core, stream, n_new, n_windows);
}

EI_IMPULSE_ERROR kws_bank_slide_live_push_device(kws_bank_slide_live *sl, size_t n, const size_t *streams, const int16_t *pcm,
                                                 const size_t *offsets, const size_t *lengths, float *const *scores, float *features,
                                                 size_t *n_windows, void *stream)
{
    if (!sl) return fail(KWS_ERROR_BAD_ARGUMENT, "null argument");
    kws_bank *b = sl->b;
    if (scores && bank_wants_nothing(b, scores, features)) return fail(KWS_ERROR_BAD_ARGUMENT, "no output requested: every scores[k] and features are NULL");
    HIP_TRY(hipSetDevice(b->device));
    hipStream_t s = (hipStream_t)stream;
    BankUse use(b, s, true);
    BankWindows ctx{ b, scores, features };
    return kws_slide_live_run(sl->core, n, streams, pcm, offsets, lengths, scores, n_windows, bank_max_labels(b), 0, 0, bank_window_finish, &ctx, s);
}

EI_IMPULSE_ERROR kws_bank_run_classifier_ragged_device(kws_bank *b, const int16_t *pcm, const size_t *offsets, const size_t *lengths, size_t B,
                                                       float *const *scores, float *features, void *stream)
{
    if (!b || !scores) return fail(KWS_ERROR_BAD_ARGUMENT, "null argument");
    if (bank_wants_nothing(b, scores, features)) return fail(KWS_ERROR_BAD_ARGUMENT, "no output requested: every scores[k] and features are NULL");
    if (B >= ((size_t)1 << 31)) return fail(KWS_ERROR_BAD_ARGUMENT, "batch too large");
    if (B == 0) return EI_IMPULSE_OK;
    HIP_TRY(hipSetDevice(b->device));
    hipStream_t s = (hipStream_t)stream;
    BankUse use(b, s, true);
    float *f = features;
    if (!f) {
        EI_IMPULSE_ERROR e = grow_buffer(&b->feat, &b->feat_cap, B * (size_t)b->m[0]->model.nn_input_frame_size);
        if (e) return e;
        f = b->feat;
    }
    BankWindows ctx{ b, scores, features };
    return kws_ragged_run(b->m[0], pcm, offsets, lengths, B, f, nullptr, 0, 0, bank_ragged_finish, &ctx, s);
}

#pragma GCC visibility pop
}
