// kws_slide.cpp -- every one-shot window of whole recordings at any hop (kws_slide_window_count, kws_slide_plan,
// kws_slide_recordings_device; contract in include/kws/kws.h).
//
// Window w of a recording is its samples [w hop, w hop + clip), and its feature matrix is what run_classifier() computes for that clip.
// Frames are independent but for pre-emphasis' predecessor of a window's FIRST sample, which wraps to the window's last sample
// (processing.hpp:77-120): frame f >= 1 of window w depends only on the samples from w hop + f stride - 1 on, so it is THE cepstral row of
// that position of the recording, whichever window reads it.  With g = gcd(hop, stride) every frame starts at a multiple of g:
//   position (w hop + f stride) / g = phase + j (stride / g),  phase < stride / g;
// the positions of one phase are frames one stride apart -- a run the spectral kernels take as one long window, cut into items of nfi frames
// with the sample before the item as its wrap.  Windows w, w + phases, w + 2 phases ... share a phase (hop / g and stride / g are coprime),
// so a recording has min(W, phases) SLOTS, slot t = w % phases, and window i of a slot starts hop / g rows after window i - 1 of it.
//   shared path:  1. the runs of every slot through spectral_device (kws_slide_stage_kernel: aligned items + wrap) into one row array;
//                 2. per chunk of windows: frame 0 of each window, nfi windows per item (kws_slide_stage_first_kernel), through
//                    spectral_device with the item's frame pitch as the plan's stride; MFE block: no pre-emphasis, frame 0 is shared too;
//                 3. windows gathered into [chunk][F] (kws_slide_gather_kernel);
//   direct path:  per chunk, the windows staged as aligned clips and the handle's own plan through spectral_device into [chunk][F];
//   both:         the finishing step of the caller of kws_slide_run: for kws_slide_recordings_device, cmvn_nn_device (cmvn_nn_fast_device in
//                 KWS_MODE_FAST) writes the chunk's scores and features in place; a bank (kws_bank.cpp) runs cmvnw once, then every member.
// Where hop / g > frames per window - 1 the windows of a slot do not touch: each is a segment of its own (nothing is shared, and AUTO
// takes the direct path).
#include "kws_internal.h"

int kws_launch_slide_stage(const int16_t *pcm, const long long *src, const long long *end, const long long *ibase, int n_slots, long long item0,
                           int n_items, long long ips, long long seg_pitch, long long item_adv, int item_len, int has_wrap, int16_t *stage, float *wrap,
                           hipStream_t stream);
int kws_launch_slide_stage_first(const int16_t *pcm, const long long *off, const long long *wbase, int n_rec, long long win0, int n_win, int nfi, int S1,
                                 int used, long long hop, int clip, int16_t *stage, float *wrap, hipStream_t stream);
int kws_launch_slide_gather(const float *rows, const float *first, const long long *wbase, const long long *sbase, const long long *ibase, int n_rec,
                            long long win0, int n_win, long long phases, long long pitch, int nfi, int pre, int nf, int ncols, float *out,
                            hipStream_t stream);
int kws_launch_scan_count(int *flags, int *flags2, int *acc, int finish, hipStream_t stream);      // kws_scan_kernels.hip

// bounded scratch of one call (include/kws/kws.h states the bound): staged items and gathered windows, as the scan's
static const size_t kSlideStageBytes = (size_t)32 << 20;
static const size_t kSlideWindowBytes = (size_t)64 << 20;
static const size_t kSlideMaxItems = 16384, kSlideMaxWindows = 32768;
static const int kSlideItemFrames = 48;            // frames per item: six eight-frame passes of kws_mfcc8_kernel, whole chunks of the general kernels
static const size_t kSlideMaxSamples = (size_t)1 << 56;      // per recording, offset and hop: beyond it the arguments are refused
static const size_t kSlideMaxTotal = (size_t)1 << 40;        // windows x labels of one call, as the scan's

struct KwsSlideScratch {
    int16_t *stage = nullptr;
    float *wrap = nullptr, *win = nullptr, *rows = nullptr, *first = nullptr;
    long long *meta = nullptr;
    int *acc = nullptr;
    size_t stage_cap = 0, wrap_cap = 0, win_cap = 0, rows_cap = 0, first_cap = 0, meta_cap = 0, acc_cap = 0;
};

static void slide_release(kws_handle *h)
{
    KwsSlideScratch *s = h->slide;
    if (!s) return;
    for (void *p : { (void *)s->stage, (void *)s->wrap, (void *)s->win, (void *)s->rows, (void *)s->first, (void *)s->meta, (void *)s->acc })
        if (p) (void)hipFree(p);
    delete s;
    h->slide = nullptr;
}

static size_t gcd_sz(size_t a, size_t b) { while (b) { const size_t t = a % b; a = b; b = t; } return a; }

// what depends on the model and the hop alone
struct SlideGeom {
    size_t clip = 0, hop = 0;
    int nf = 0, stride = 0, ncols = 0, used = 0;
    int pre = 0;                   // 1: pre-emphasis block, frame 0 is per window; 0: MFE block
    int run = 0;                   // shared rows per window: nf - pre
    size_t hg = 0, phases = 0;     // hop / g, stride / g
    bool touching = false;         // the windows of a slot overlap or abut: a slot is one run
    int nfi = 0;                   // frames per item
    size_t ips = 0, pitch = 0;     // items per segment (one run: no limit); rows from a slot's window to its next
    size_t windows(size_t n) const { return n < clip ? 0 : (n - clip) / hop + 1; }
    size_t slots(size_t W) const { return run > 0 ? std::min(W, phases) : 0; }
    size_t slot_windows(size_t W, size_t t) const { return (W - t + phases - 1) / phases; }
    size_t slot_rows(size_t nt) const { return touching ? (nt - 1) * hg + (size_t)run : nt * (size_t)run; }
    size_t slot_items(size_t nt) const { return touching ? (slot_rows(nt) + nfi - 1) / nfi : nt * ips; }
};

static void slide_geom(const kws_handle *h, size_t hop, SlideGeom *G)
{
    const KwsDspPlan &P = h->dsp;
    G->clip = h->model.raw_sample_count;
    G->hop = hop;
    G->nf = P.n_frames; G->stride = P.frame_stride; G->ncols = P.n_cepstral;
    G->used = std::min(P.frame_len, P.fft_len);
    G->pre = h->model.dsp.block == DSP_BLOCK_MFE ? 0 : 1;
    G->run = G->nf - G->pre;
    const size_t g = gcd_sz(hop, (size_t)G->stride);
    G->hg = hop / g;
    G->phases = (size_t)G->stride / g;
    G->touching = G->hg <= (size_t)G->run;
    G->nfi = std::max(1, std::min(kSlideItemFrames, G->nf));
    G->ips = G->touching ? (size_t)1 << 62 : ((size_t)G->run + G->nfi - 1) / G->nfi;
    G->pitch = G->touching ? G->hg : G->ips * (size_t)G->nfi;
}

// the AUTO rule: the shared path where it computes fewer rows than the direct one
static int slide_pick(int flags, const kws_slide_plan_info &I)
{
    if (flags == KWS_SLIDE_DIRECT || flags == KWS_SLIDE_SHARED) return flags;
    return I.rows_shared + I.rows_first < I.rows_direct ? KWS_SLIDE_SHARED : KWS_SLIDE_DIRECT;
}

static EI_IMPULSE_ERROR slide_check(const kws_handle *h, size_t hop, int flags)
{
    if (!h) return fail(KWS_ERROR_BAD_ARGUMENT, "null argument");
    if (hop == 0 || hop > kSlideMaxSamples) return fail(KWS_ERROR_BAD_ARGUMENT, "hop of %zu samples", hop);
    if (flags != KWS_SLIDE_AUTO && flags != KWS_SLIDE_DIRECT && flags != KWS_SLIDE_SHARED) return fail(KWS_ERROR_BAD_ARGUMENT, "unknown flags %d", flags);
    return EI_IMPULSE_OK;
}

static EI_IMPULSE_ERROR slide_plan(const kws_handle *h, const size_t *lengths, size_t R, size_t hop, int flags, SlideGeom *G, kws_slide_plan_info *I)
{
    EI_IMPULSE_ERROR e = slide_check(h, hop, flags);
    if (e) return e;
    if (R > 0 && !lengths) return fail(KWS_ERROR_BAD_ARGUMENT, "null argument");
    if (R > 0x3fffffff) return fail(KWS_ERROR_BAD_ARGUMENT, "too many recordings");
    slide_geom(h, hop, G);
    memset(I, 0, sizeof(*I));
    I->phases = (int)G->phases;
    for (size_t r = 0; r < R; ++r) {
        if (lengths[r] > kSlideMaxSamples) return fail(KWS_ERROR_BAD_ARGUMENT, "recording of %zu samples", lengths[r]);
        const size_t W = G->windows(lengths[r]);
        if (W > kSlideMaxTotal || (I->n_windows += W) > kSlideMaxTotal || I->n_windows * h->model.labels.size() > kSlideMaxTotal)
            return fail(KWS_ERROR_BAD_ARGUMENT, "too many windows");
        for (size_t t = 0, T = G->slots(W); t < T; ++t) I->rows_shared += G->slot_rows(G->slot_windows(W, t));
    }
    I->rows_first = G->pre ? I->n_windows : 0;
    I->rows_direct = I->n_windows * (size_t)G->nf;
    I->path = slide_pick(flags, *I);
    return EI_IMPULSE_OK;
}

// The finishing step of kws_slide_recordings_device itself: cmvnw + the handle's network in the handle's mode, chunk by chunk (h->mu held)
struct SlideOwn {
    kws_handle *h;
    float *scores, *features;
    bool started = false, fast = false, count = false;
};
static EI_IMPULSE_ERROR slide_own_finish(void *ctx, float *win, size_t n, size_t g0, hipStream_t st)
{
    SlideOwn &o = *(SlideOwn *)ctx;
    kws_handle *h = o.h;
    const Model &m = h->model;
    const size_t F = m.nn_input_frame_size, C = m.labels.size();
    KwsSlideScratch &S = *h->slide;
    int rc = 0;
    if (!o.started) {
        o.started = true;
        o.fast = h->mode == KWS_MODE_FAST && h->fast_plain_ok;
        o.count = o.fast && m.dsp.block != DSP_BLOCK_MFE;          // the MFE block's fast form is its exact one: no guard, no counts
        if (o.count) HIP_TRY(hipMemsetAsync(S.acc, 0, sizeof(int), st));
    }
    if (n == 0) {                                                  // after the last chunk
        if (o.count && (rc = kws_launch_scan_count(h->d_flags, h->d_flags2, S.acc, 1, st)))
            return fail(KWS_ERROR_HIP, "count kernel launch failed: %s", hipGetErrorString((hipError_t)rc));
        return EI_IMPULSE_OK;
    }
    // slide calls write no logits tap (out of the tap's [B][labels] shape): the tap is set aside for the step
    struct TapAside {
        kws_handle *h; float *t;
        ~TapAside() { h->tap_logits = t; }
    } tap_aside{ h, h->tap_logits };
    h->tap_logits = nullptr;
    EI_IMPULSE_ERROR e;
    float *f = o.features ? o.features + g0 * F : nullptr;
    if (o.fast) e = cmvn_nn_fast_device(h, win, n, o.scores + g0 * C, st, 0, 0, f);
    else e = cmvn_nn_device(h, win, n, f, nullptr, o.scores + g0 * C, nullptr, nullptr, nullptr, st);
    if (e) return e;
    if (o.count && (rc = kws_launch_scan_count(h->d_flags, h->d_flags2, S.acc, 0, st)))
        return fail(KWS_ERROR_HIP, "count kernel launch failed: %s", hipGetErrorString((hipError_t)rc));
    return EI_IMPULSE_OK;
}

// The slide: argument checks, staging, cepstral rows and gathering for the handle's DSP block; every chunk of gathered windows
// (win [n][F] cepstra before cmvnw, the call's windows g0 .. g0 + n - 1) goes to finish(), which is called once more with n == 0 after
// the last chunk.  take_lock == 0: the caller holds h->mu (kws_bank.cpp, which holds every member's).
EI_IMPULSE_ERROR kws_slide_run(kws_handle *h, const int16_t *pcm, const size_t *offsets, const size_t *lengths, size_t R, size_t hop_samples, int flags,
                               int take_lock, kws_slide_finish_fn finish, void *ctx, hipStream_t st)
{
    if (R > 0 && (!pcm || !offsets || !lengths)) return fail(KWS_ERROR_BAD_ARGUMENT, "null argument");
    SlideGeom G;
    kws_slide_plan_info I;
    EI_IMPULSE_ERROR e = slide_plan(h, lengths, R, hop_samples, flags, &G, &I);
    if (e) return e;
    if (I.n_windows == 0) return EI_IMPULSE_OK;
    const bool shared = I.path == KWS_SLIDE_SHARED;
    // the recordings that produce windows: where they lie, where their windows and slots go; per slot its first sample and its items
    std::vector<long long> off, end, wbase(1, 0), sbase(1, 0), ssrc, send, ibase(1, 0);
    for (size_t r = 0; r < R; ++r) {
        const size_t W = G.windows(lengths[r]);
        if (!W) continue;
        if (offsets[r] > kSlideMaxSamples) return fail(KWS_ERROR_BAD_ARGUMENT, "recording at sample %zu", offsets[r]);
        off.push_back((long long)offsets[r]);
        end.push_back((long long)(offsets[r] + lengths[r]));
        wbase.push_back(wbase.back() + (long long)W);
        const size_t T = shared ? G.slots(W) : 0;
        for (size_t t = 0; t < T; ++t) {
            ssrc.push_back((long long)(offsets[r] + t * G.hop + (size_t)G.pre * G.stride));      // frame `pre` of window t
            send.push_back(end.back());
            ibase.push_back(ibase.back() + (long long)G.slot_items(G.slot_windows(W, t)));
        }
        sbase.push_back(sbase.back() + (long long)T);
    }
    const size_t A = off.size(), NS = ssrc.size(), n_win = I.n_windows, n_items = (size_t)ibase.back();
    if (NS > 0x3fffffff) return fail(KWS_ERROR_BAD_ARGUMENT, "too many recordings x phases");
    const size_t F = h->model.nn_input_frame_size;
    const int ncols = G.ncols, nfi = G.nfi;
    HIP_TRY(hipSetDevice(h->device));
    std::unique_lock<std::mutex> lk(h->mu, std::defer_lock);
    if (take_lock) lk.lock();
    if (!h->slide) { h->slide = new KwsSlideScratch(); h->slide_release = slide_release; }
    KwsSlideScratch &S = *h->slide;
    // staged items: a run item is nfi frames one stride apart; a frame-0 item is nfi slots of S1 samples; a direct item is a window
    const size_t run_len = (((size_t)(nfi - 1) * G.stride + (size_t)std::max(G.used, 1)) + 7) & ~(size_t)7;
    const size_t S1 = ((size_t)G.used + 1 + 7) & ~(size_t)7, first_len = (size_t)nfi * S1;
    const size_t win_chunk = std::min(std::max<size_t>(1, std::min(kSlideMaxWindows, kSlideWindowBytes / (F * sizeof(float)))), n_win);
    const size_t run_cap = std::max<size_t>(1, std::min(kSlideMaxItems, kSlideStageBytes / (run_len * sizeof(int16_t))));
    const size_t first_cap = std::max<size_t>(1, std::min(kSlideMaxItems, kSlideStageBytes / (first_len * sizeof(int16_t))));
    const size_t clip_cap = std::max<size_t>(1, std::min(kSlideMaxItems, kSlideStageBytes / (G.clip * sizeof(int16_t))));
    const size_t first_items = (win_chunk + nfi - 1) / nfi;
    size_t stage_need, wrap_need;
    if (shared) {
        stage_need = std::max(std::min(run_cap, std::max<size_t>(n_items, 1)) * run_len, G.pre ? std::min(first_cap, first_items) * first_len : 0);
        wrap_need = std::max(std::min(run_cap, std::max<size_t>(n_items, 1)), std::min(first_cap, first_items));
    } else {
        stage_need = std::min(clip_cap, win_chunk) * G.clip;
        wrap_need = 1;
    }
    const size_t n_meta = 2 * A + 2 * (A + 1) + 2 * NS + (NS + 1);
    if ((e = grow_buffer(&S.stage, &S.stage_cap, stage_need)) || (e = grow_buffer(&S.wrap, &S.wrap_cap, wrap_need)) ||
        (e = grow_buffer(&S.win, &S.win_cap, win_chunk * F)) || (e = grow_buffer(&S.rows, &S.rows_cap, std::max<size_t>(n_items * nfi * ncols, 1))) ||
        (e = grow_buffer(&S.first, &S.first_cap, shared && G.pre ? first_items * nfi * ncols : 1)) || (e = grow_buffer(&S.meta, &S.meta_cap, n_meta)) ||
        (e = grow_buffer(&S.acc, &S.acc_cap, 1)) || (e = ensure_scratch(h, win_chunk)))
        return e;
    ScratchUse use(h, st);
    // tables: off [A], end [A], wbase [A + 1], sbase [A + 1], ssrc [NS], send [NS], ibase [NS + 1].  The host copy is complete before the call goes on
    std::vector<long long> meta;
    meta.reserve(n_meta);
    for (const std::vector<long long> *v : { &off, &end, &wbase, &sbase, &ssrc, &send, &ibase }) meta.insert(meta.end(), v->begin(), v->end());
    HIP_TRY(hipMemcpyAsync(S.meta, meta.data(), meta.size() * sizeof(long long), hipMemcpyHostToDevice, st));
    HIP_TRY(hipStreamSynchronize(st));
    const long long *d_off = S.meta, *d_end = d_off + A, *d_wbase = d_end + A, *d_sbase = d_wbase + A + 1, *d_ssrc = d_sbase + A + 1, *d_send = d_ssrc + NS,
                    *d_ibase = d_send + NS;
    int rc = 0;
    if (shared) {
        // 1. the runs: the spectral launches of the one-shot path on items of nfi frames, each with the sample before it as its x[-1]
        KwsDspPlan PR = h->dsp;
        PR.n_samples = (int)run_len;
        PR.n_frames = nfi;
        PR.wrap_index = PR.n_samples - 1;
        for (size_t g0 = 0; g0 < n_items; g0 += run_cap) {
            const int n = (int)std::min(run_cap, n_items - g0);
            rc = kws_launch_slide_stage(pcm, d_ssrc, d_send, d_ibase, (int)NS, (long long)g0, n, (long long)G.ips, (long long)(G.phases * G.hop),
                                        (long long)nfi * G.stride, (int)run_len, G.pre, S.stage, S.wrap, st);
            if (rc) return fail(KWS_ERROR_HIP, "slide staging kernel launch failed: %s", hipGetErrorString((hipError_t)rc));
            if ((e = spectral_device(h, PR, S.stage, 0, n, S.rows + g0 * nfi * ncols, S.wrap, st, nfi * ncols))) return e;
        }
    }
    KwsDspPlan PF = h->dsp;                                 // frame 0 of nfi windows per item: the frames S1 samples apart
    PF.frame_stride = (int)S1;
    PF.n_samples = (int)first_len;
    PF.n_frames = nfi;
    PF.wrap_index = PF.n_samples - 1;
    // 2. windows in chunks through the finishing step (cmvnw + the network)
    for (size_t g0 = 0; g0 < n_win; g0 += win_chunk) {
        const int n = (int)std::min(win_chunk, n_win - g0);
        if (shared) {
            for (size_t i0 = 0; G.pre && i0 < (size_t)n; i0 += first_cap * nfi) {
                const int nw = (int)std::min(first_cap * nfi, (size_t)n - i0), ni = (nw + nfi - 1) / nfi;
                rc = kws_launch_slide_stage_first(pcm, d_off, d_wbase, (int)A, (long long)(g0 + i0), nw, nfi, (int)S1, G.used, (long long)G.hop, (int)G.clip,
                                                  S.stage, S.wrap, st);
                if (rc) return fail(KWS_ERROR_HIP, "slide staging kernel launch failed: %s", hipGetErrorString((hipError_t)rc));
                if ((e = spectral_device(h, PF, S.stage, 0, ni, S.first + i0 * ncols, S.wrap, st, nfi * ncols))) return e;
            }
            rc = kws_launch_slide_gather(S.rows, S.first, d_wbase, d_sbase, d_ibase, (int)A, (long long)g0, n, (long long)G.phases, (long long)G.pitch, nfi,
                                         G.pre, G.nf, ncols, S.win, st);
            if (rc) return fail(KWS_ERROR_HIP, "slide gather kernel launch failed: %s", hipGetErrorString((hipError_t)rc));
        } else {
            // the windows as aligned clips (recordings as slots, windows as their items, one hop apart), then the handle's own plan
            for (size_t i0 = 0; i0 < (size_t)n; i0 += clip_cap) {
                const int nw = (int)std::min(clip_cap, (size_t)n - i0);
                rc = kws_launch_slide_stage(pcm, d_off, d_end, d_wbase, (int)A, (long long)(g0 + i0), nw, 1, (long long)G.hop, 0, (int)G.clip, 0, S.stage,
                                            nullptr, st);
                if (rc) return fail(KWS_ERROR_HIP, "slide staging kernel launch failed: %s", hipGetErrorString((hipError_t)rc));
                if ((e = spectral_device(h, h->dsp, S.stage, 0, nw, S.win + i0 * F, nullptr, st, 0))) return e;
            }
        }
        if ((e = finish(ctx, S.win, (size_t)n, g0, st))) return e;
    }
    return finish(ctx, S.win, 0, n_win, st);
}

extern "C" {
#pragma GCC visibility push(default)

int kws_frame_stride_samples(const kws_handle *h) { return h->dsp.frame_stride; }

EI_IMPULSE_ERROR kws_slide_window_count(const kws_handle *h, size_t n_samples, size_t hop_samples, size_t *n_windows)
{
    if (!h || !n_windows) return fail(KWS_ERROR_BAD_ARGUMENT, "null argument");
    *n_windows = 0;
    EI_IMPULSE_ERROR e = slide_check(h, hop_samples, KWS_SLIDE_AUTO);
    if (e) return e;
    if (n_samples > kSlideMaxSamples) return fail(KWS_ERROR_BAD_ARGUMENT, "recording of %zu samples", n_samples);
    const size_t clip = h->model.raw_sample_count;
    *n_windows = n_samples < clip ? 0 : (n_samples - clip) / hop_samples + 1;
    return EI_IMPULSE_OK;
}

EI_IMPULSE_ERROR kws_slide_plan(const kws_handle *h, const size_t *lengths, size_t R, size_t hop_samples, int flags, kws_slide_plan_info *out)
{
    if (!h || !out) return fail(KWS_ERROR_BAD_ARGUMENT, "null argument");
    SlideGeom G;
    return slide_plan(h, lengths, R, hop_samples, flags, &G, out);
}

EI_IMPULSE_ERROR kws_slide_recordings_device(kws_handle *h, const int16_t *pcm, const size_t *offsets, const size_t *lengths, size_t R,
                                             size_t hop_samples, int flags, float *scores, float *features, void *stream)
{
    if (!h || !scores) return fail(KWS_ERROR_BAD_ARGUMENT, "null argument");
    SlideOwn own{ h, scores, features };
    return kws_slide_run(h, pcm, offsets, lengths, R, hop_samples, flags, 1, slide_own_finish, &own, (hipStream_t)stream);
}

#pragma GCC visibility pop
}
