// kws_windows.h -- the host core of the four window pipelines: recording scans (kws_scan.cpp), live continuous streams (kws_live.cpp), one-shot
// windows over recordings (kws_slide.cpp) and live one-shot windows (kws_slide_live.cpp).  Each stages items for the spectral kernels, gathers
// windows in bounded chunks and finishes every chunk with cmvnw + the network; what they share is here, once: the scratch and its bounds, the
// table upload, the finishing step, the fast mode's counts over chunks, the skeleton of a live session and the slide's geometry.  Header-only
// (static inline): every unit that includes it carries what it uses, so no unit list changes.  Include it after kws_internal.h.
#pragma once
#include "kws_internal.h"

#include <initializer_list>

int kws_launch_scan_count(int *flags, int *flags2, int *acc, int finish, hipStream_t stream);      // kws_scan_kernels.hip

// ---- bounded scratch of one call (include/kws/kws.h states the bounds): staged items and gathered windows ----------------------------------
static const size_t kWindowStageBytes = (size_t)32 << 20;
static const size_t kWindowGatherBytes = (size_t)64 << 20;
static const size_t kWindowMaxItems = 16384, kWindowMaxWindows = 32768;
static const int kWindowItemFrames = 48;           // frames per slide item: six eight-frame passes of kws_mfcc8_kernel, whole chunks of the general kernels
static const unsigned long long kLiveMaxSamples = 1ull << 60;           // samples of one live stream between starts (positions stay in long long)

// items of item_samples int16 samples staged at once
static inline size_t kws_window_item_cap(size_t item_samples)
{
    return std::max<size_t>(1, std::min(kWindowMaxItems, kWindowStageBytes / (item_samples * sizeof(int16_t))));
}
// windows of F floats gathered at once, of a call with n_win windows
static inline size_t kws_window_chunk(size_t F, size_t n_win)
{
    return std::min(std::max<size_t>(1, std::min(kWindowMaxWindows, kWindowGatherBytes / (F * sizeof(float)))), std::max<size_t>(n_win, 1));
}

struct KwsWindowScratch {
    int16_t *stage = nullptr;
    float *wrap = nullptr, *win = nullptr, *rows = nullptr;
    long long *meta = nullptr;
    int *acc = nullptr;
    size_t stage_cap = 0, wrap_cap = 0, win_cap = 0, rows_cap = 0, meta_cap = 0, acc_cap = 0;

    // grows every buffer to the call's needs (elements), and the handle's own scratch to win_chunk windows
    EI_IMPULSE_ERROR reserve(kws_handle *h, size_t stage_n, size_t wrap_n, size_t win_n, size_t rows_n, size_t meta_n, size_t win_chunk)
    {
        EI_IMPULSE_ERROR e;
        if ((e = grow_buffer(&stage, &stage_cap, stage_n)) || (e = grow_buffer(&wrap, &wrap_cap, wrap_n)) || (e = grow_buffer(&win, &win_cap, win_n)) ||
            (e = grow_buffer(&rows, &rows_cap, rows_n)) || (e = grow_buffer(&meta, &meta_cap, meta_n)) || (e = grow_buffer(&acc, &acc_cap, 1)))
            return e;
        return ensure_scratch(h, win_chunk);
    }
    void release()
    {
        for (void *p : { (void *)stage, (void *)wrap, (void *)win, (void *)rows, (void *)meta, (void *)acc })
            if (p) (void)hipFree(p);
        *this = KwsWindowScratch();
    }
};

// The call's tables, packed in order into S.meta.  The host copy is complete before the call goes on
static inline EI_IMPULSE_ERROR kws_upload_tables(KwsWindowScratch &S, std::initializer_list<const std::vector<long long> *> tables, hipStream_t st)
{
    size_t total = 0;
    for (const std::vector<long long> *v : tables) total += v->size();
    std::vector<long long> meta;
    meta.reserve(total);
    for (const std::vector<long long> *v : tables) meta.insert(meta.end(), v->begin(), v->end());
    HIP_TRY(hipMemcpyAsync(S.meta, meta.data(), meta.size() * sizeof(long long), hipMemcpyHostToDevice, st));
    HIP_TRY(hipStreamSynchronize(st));
    return EI_IMPULSE_OK;
}

// The finishing step of one chunk of gathered windows (win [n][feature_count] cepstra before cmvnw, device; h->mu held): cmvnw + the handle's
// network, through the fast forms behind the guard when `fast`; scores [n][labels] and the optional features [n][feature_count] are written in
// place.  Such calls write no logits tap (out of the tap's [B][labels] shape): it is set aside for the step.
static inline EI_IMPULSE_ERROR kws_finish_window_chunk(kws_handle *h, const float *win, size_t n, float *scores, float *features, bool fast, hipStream_t s)
{
    struct TapAside {
        kws_handle *h; float *t;
        ~TapAside() { h->tap_logits = t; }
    } tap_aside{ h, h->tap_logits };
    h->tap_logits = nullptr;
    if (fast) return cmvn_nn_fast_device(h, win, n, scores, s, 0, 0, features);
    return cmvn_nn_device(h, win, n, features, nullptr, scores, nullptr, nullptr, nullptr, s);
}

// KWS_MODE_FAST over the chunks of one call: every chunk's launch resets the guard's two lists, so their counts are added up in `acc` chunk by
// chunk and written back at the end -- kws_fast_fallback_count / kws_fast_exact_count then describe the whole call.
struct KwsChunkCounts {
    kws_handle *h;
    bool fast, on;                 // the chunks take the fast forms; their counts are kept
    int *acc = nullptr;
    explicit KwsChunkCounts(kws_handle *h_) : h(h_), fast(h_->mode == KWS_MODE_FAST && h_->fast_plain_ok), on(wanted(h_)) {}
    static bool wanted(const kws_handle *h)
    {
        // the MFE block's fast form is its exact one: no guard, no counts
        return h->mode == KWS_MODE_FAST && h->fast_plain_ok && h->model.dsp.block != DSP_BLOCK_MFE;
    }
    EI_IMPULSE_ERROR launch(int finish, hipStream_t st)
    {
        int rc = on ? kws_launch_scan_count(h->d_flags, h->d_flags2, acc, finish, st) : 0;
        return rc ? fail(KWS_ERROR_HIP, "count kernel launch failed: %s", hipGetErrorString((hipError_t)rc)) : EI_IMPULSE_OK;
    }
    // before the first of the call's n_win windows (none: nothing to add up, nothing is launched)
    EI_IMPULSE_ERROR begin(int *acc_, size_t n_win, hipStream_t st)
    {
        acc = acc_;
        on = on && n_win > 0;
        if (on) HIP_TRY(hipMemsetAsync(acc, 0, sizeof(int), st));
        return EI_IMPULSE_OK;
    }
    EI_IMPULSE_ERROR chunk(hipStream_t st) { return launch(0, st); }
    EI_IMPULSE_ERROR end(hipStream_t st) { return launch(1, st); }
    // a live push with no window: kws_fast_fallback_count / kws_fast_exact_count describe the last push, none of whose windows was handed back
    static EI_IMPULSE_ERROR none(kws_handle *h, hipStream_t st)
    {
        HIP_TRY(hipMemsetAsync(h->d_flags, 0, sizeof(int), st));
        HIP_TRY(hipMemsetAsync(h->d_flags2, 0, sizeof(int), st));
        return EI_IMPULSE_OK;
    }
};

// ---- the skeleton of a live session (kws_live, kws_slide_live): S streams on one handle, host mirrors of each stream's counts, state in HBM ---
struct KwsLiveSession {
    kws_handle *h = nullptr;
    size_t S = 0;
    std::vector<unsigned long long> n;     // per stream: samples since its start
    std::vector<unsigned long long> m2;    // per stream: the session's second count (finished slices / shared positions computed)
    int16_t *carry = nullptr;              // state in HBM: carried samples, retained cepstral rows
    float *kept = nullptr;
    KwsWindowScratch scratch;              // per-push scratch, grown on demand

    void open(kws_handle *h_, size_t S_) { h = h_; S = S_; n.assign(S_, 0); m2.assign(S_, 0); }
    void free_device()
    {
        if (carry) (void)hipFree(carry);
        if (kept) (void)hipFree(kept);
        carry = nullptr; kept = nullptr;
        scratch.release();
    }
    // the argument checks of a push of n_e entries (h->mu held), before any state changes
    EI_IMPULSE_ERROR check_push(size_t n_e, const size_t *streams, const int16_t *pcm, const size_t *offsets, const size_t *lengths, const size_t *n_windows,
                                const float *scores) const
    {
        if (n_e > 0 && (!streams || !lengths || !n_windows || !scores)) return fail(KWS_ERROR_BAD_ARGUMENT, "null argument");
        if (n_e > S) return fail(KWS_ERROR_BAD_ARGUMENT, "%zu entries for %zu streams", n_e, S);
        std::vector<char> named(S, 0);
        bool any_samples = false;
        for (size_t i = 0; i < n_e; ++i) {
            const size_t s = streams[i];
            if (s >= S) return fail(KWS_ERROR_BAD_ARGUMENT, "entry %zu: stream %zu of %zu", i, s, S);
            if (named[s]) return fail(KWS_ERROR_BAD_ARGUMENT, "entry %zu: stream %zu named twice", i, s);
            named[s] = 1;
            if (lengths[i] > kLiveMaxSamples - n[s]) return fail(KWS_ERROR_BAD_ARGUMENT, "entry %zu: too many samples", i);
            any_samples = any_samples || lengths[i] > 0;
        }
        if (any_samples && (!pcm || !offsets)) return fail(KWS_ERROR_BAD_ARGUMENT, "null argument");
        return EI_IMPULSE_OK;
    }
    // all streams (streams == NULL), or a checked list of them, back to their start
    EI_IMPULSE_ERROR reset(const size_t *streams, size_t n_s)
    {
        if (n_s > 0 && !streams) return fail(KWS_ERROR_BAD_ARGUMENT, "null argument");
        std::lock_guard<std::mutex> lk(h->mu);
        if (!streams) {
            std::fill(n.begin(), n.end(), 0);
            std::fill(m2.begin(), m2.end(), 0);
            return EI_IMPULSE_OK;
        }
        for (size_t i = 0; i < n_s; ++i)
            if (streams[i] >= S) return fail(KWS_ERROR_BAD_ARGUMENT, "stream %zu of %zu", streams[i], S);
        for (size_t i = 0; i < n_s; ++i) n[streams[i]] = m2[streams[i]] = 0;
        return EI_IMPULSE_OK;
    }
    // the windows a push of n_new samples to `stream` would return: rule(samples before, samples after), under the handle's lock
    template <typename Rule> EI_IMPULSE_ERROR window_count(size_t stream, size_t n_new, size_t *n_windows, Rule rule) const
    {
        if (!n_windows) return fail(KWS_ERROR_BAD_ARGUMENT, "null argument");
        *n_windows = 0;
        if (stream >= S) return fail(KWS_ERROR_BAD_ARGUMENT, "stream %zu of %zu", stream, S);
        std::lock_guard<std::mutex> lk(h->mu);
        const unsigned long long n0 = n[stream];
        if (n_new > kLiveMaxSamples - n0) return fail(KWS_ERROR_BAD_ARGUMENT, "stream %zu: too many samples", stream);
        *n_windows = rule(n0, n0 + n_new);
        return EI_IMPULSE_OK;
    }
};

// destroys a session (a KwsLiveSession with a free_device() of its own) once the handle's latest call has ended
template <typename Session> static inline void kws_session_destroy(Session *s)
{
    if (!s) return;
    kws_handle *h = s->h;
    std::lock_guard<std::mutex> lk(h->mu);
    (void)hipSetDevice(h->device);
    // every push brackets its work with ScratchUse: the handle's event marks the end of the latest call, this session's last push included
    if (h->scratch_used && h->scratch_ev) (void)hipEventSynchronize(h->scratch_ev);
    s->free_device();
    delete s;
}

// ---- the slide's geometry: what depends on the model and the hop alone (kws_slide.cpp's header comment has the argument) ---------------------
struct SlideGeom {
    size_t clip = 0, hop = 0;
    int nf = 0, stride = 0, ncols = 0, used = 0;
    int pre = 0;                   // 1: pre-emphasis block, frame 0 is per window; 0: MFE block
    int run = 0;                   // shared rows per window: nf - pre
    size_t hg = 0, phases = 0;     // hop / g, stride / g
    bool touching = false;         // the windows of a slot overlap or abut: a slot is one run
    int nfi = 0;                   // frames per item
    size_t ips = 0, pitch = 0;     // items per segment (one run: no limit); rows from a slot's window to its next
    size_t S1 = 0;                 // samples per frame of a frame-0 item: the frame and, before the next one, its predecessor sample
    size_t windows(unsigned long long n) const { return n < clip ? 0 : (size_t)((n - clip) / hop) + 1; }
    size_t slots(size_t W) const { return run > 0 ? std::min(W, phases) : 0; }
    size_t slot_windows(size_t W, size_t t) const { return (W - t + phases - 1) / phases; }
    size_t slot_rows(size_t nt) const { return touching ? (nt - 1) * hg + (size_t)run : nt * (size_t)run; }
    size_t slot_items(size_t nt) const { return touching ? (slot_rows(nt) + nfi - 1) / nfi : nt * ips; }
    // the handle's plan for items of nfi independent frames S1 samples apart, each with its predecessor in the sample before it
    KwsDspPlan first_plan(const kws_handle *h) const
    {
        KwsDspPlan PF = h->dsp;
        PF.frame_stride = (int)S1;
        PF.n_samples = nfi * (int)S1;
        PF.n_frames = nfi;
        PF.wrap_index = PF.n_samples - 1;
        return PF;
    }
};

static inline void slide_geom(const kws_handle *h, size_t hop, SlideGeom *G)
{
    const KwsDspPlan &P = h->dsp;
    G->clip = h->model.raw_sample_count;
    G->hop = hop;
    G->nf = P.n_frames; G->stride = P.frame_stride; G->ncols = P.n_cepstral;
    G->used = std::min(P.frame_len, P.fft_len);
    G->pre = h->model.dsp.block == DSP_BLOCK_MFE ? 0 : 1;
    G->run = G->nf - G->pre;
    size_t g = hop, b = (size_t)G->stride;             // gcd(hop, stride)
    while (b) { const size_t t = g % b; g = b; b = t; }
    G->hg = hop / g;
    G->phases = (size_t)G->stride / g;
    G->touching = G->hg <= (size_t)G->run;
    G->nfi = std::max(1, std::min(kWindowItemFrames, G->nf));
    G->ips = G->touching ? (size_t)1 << 62 : ((size_t)G->run + G->nfi - 1) / G->nfi;
    G->pitch = G->touching ? G->hg : G->ips * (size_t)G->nfi;
    G->S1 = ((size_t)G->used + 1 + 7) & ~(size_t)7;
}
