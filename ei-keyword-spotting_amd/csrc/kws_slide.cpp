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
// Scratch and its bounds, the table upload, the finishing step, the fast counters and the geometry (SlideGeom): kws_windows.h.
#include "kws_internal.h"
#include "kws_windows.h"

int kws_launch_slide_stage(const int16_t *pcm, const long long *src, const long long *end, const long long *ibase, int n_slots, long long item0,
                           int n_items, long long ips, long long seg_pitch, long long item_adv, int item_len, int has_wrap, int16_t *stage, float *wrap,
                           hipStream_t stream);
int kws_launch_slide_stage_first(const int16_t *pcm, const long long *off, const long long *wbase, int n_rec, long long win0, int n_win, int nfi, int S1,
                                 int used, long long hop, int clip, int16_t *stage, float *wrap, hipStream_t stream);
int kws_launch_slide_gather(const float *rows, const float *first, const long long *wbase, const long long *sbase, const long long *ibase, int n_rec,
                            long long win0, int n_win, long long phases, long long pitch, int nfi, int pre, int nf, int ncols, float *out,
                            hipStream_t stream);

static const size_t kSlideMaxSamples = (size_t)1 << 56;      // per recording, offset and hop: beyond it the arguments are refused
static const size_t kSlideMaxTotal = (size_t)1 << 40;        // windows x labels of one call, as the scan's

struct KwsSlideScratch : KwsWindowScratch {
    float *first = nullptr;        // frame 0 of a chunk's windows (shared path)
    size_t first_cap = 0;
};

static void slide_release(kws_handle *h)
{
    KwsSlideScratch *s = h->slide;
    if (!s) return;
    s->release();
    if (s->first) (void)hipFree(s->first);
    delete s;
    h->slide = nullptr;
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
    float *scores, *features;
    KwsChunkCounts counts;
    bool started = false;
};
static EI_IMPULSE_ERROR slide_own_finish(void *ctx, float *win, size_t n, size_t g0, hipStream_t st)
{
    SlideOwn &o = *(SlideOwn *)ctx;
    kws_handle *h = o.counts.h;
    const size_t F = h->model.nn_input_frame_size, C = h->model.labels.size();
    EI_IMPULSE_ERROR e;
    if (!o.started) {
        o.started = true;
        if ((e = o.counts.begin(h->slide->acc, n, st))) return e;
    }
    if (n == 0) return o.counts.end(st);                           // after the last chunk
    if ((e = kws_finish_window_chunk(h, win, n, o.scores + g0 * C, o.features ? o.features + g0 * F : nullptr, o.counts.fast, st))) return e;
    return o.counts.chunk(st);
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
    const size_t first_len = (size_t)nfi * G.S1, win_chunk = kws_window_chunk(F, n_win);
    const size_t run_cap = kws_window_item_cap(run_len), first_cap = kws_window_item_cap(first_len), clip_cap = kws_window_item_cap(G.clip);
    const size_t first_items = (win_chunk + nfi - 1) / nfi;
    size_t stage_need, wrap_need;
    if (shared) {
        stage_need = std::max(std::min(run_cap, std::max<size_t>(n_items, 1)) * run_len, G.pre ? std::min(first_cap, first_items) * first_len : 0);
        wrap_need = std::max(std::min(run_cap, std::max<size_t>(n_items, 1)), std::min(first_cap, first_items));
    } else {
        stage_need = std::min(clip_cap, win_chunk) * G.clip;
        wrap_need = 1;
    }
    if ((e = S.reserve(h, stage_need, wrap_need, win_chunk * F, std::max<size_t>(n_items * nfi * ncols, 1), 2 * A + 2 * (A + 1) + 2 * NS + (NS + 1), win_chunk)) ||
        (e = grow_buffer(&S.first, &S.first_cap, shared && G.pre ? first_items * nfi * ncols : 1)))
        return e;
    ScratchUse use(h, st);
    // tables: off [A], end [A], wbase [A + 1], sbase [A + 1], ssrc [NS], send [NS], ibase [NS + 1]
    if ((e = kws_upload_tables(S, { &off, &end, &wbase, &sbase, &ssrc, &send, &ibase }, st))) return e;
    const long long *d_off = S.meta, *d_end = d_off + A, *d_wbase = d_end + A, *d_sbase = d_wbase + A + 1, *d_ssrc = d_sbase + A + 1, *d_send = d_ssrc + NS,
                    *d_ibase = d_send + NS;
    if (shared) {
        // 1. the runs: the spectral launches of the one-shot path on items of nfi frames, each with the sample before it as its x[-1]
        KwsDspPlan PR = h->dsp;
        PR.n_samples = (int)run_len;
        PR.n_frames = nfi;
        PR.wrap_index = PR.n_samples - 1;
        for (size_t g0 = 0; g0 < n_items; g0 += run_cap) {
            const int n = (int)std::min(run_cap, n_items - g0);
            KWS_LAUNCH_TRY("slide staging kernel", kws_launch_slide_stage(pcm, d_ssrc, d_send, d_ibase, (int)NS, (long long)g0, n, (long long)G.ips, (long long)(G.phases * G.hop),
                                                                          (long long)nfi * G.stride, (int)run_len, G.pre, S.stage, S.wrap, st));
            if ((e = spectral_device(h, PR, S.stage, 0, n, S.rows + g0 * nfi * ncols, S.wrap, st, nfi * ncols))) return e;
        }
    }
    const KwsDspPlan PF = G.first_plan(h);                 // frame 0 of nfi windows per item: the frames S1 samples apart
    // 2. windows in chunks through the finishing step (cmvnw + the network)
    for (size_t g0 = 0; g0 < n_win; g0 += win_chunk) {
        const int n = (int)std::min(win_chunk, n_win - g0);
        if (shared) {
            for (size_t i0 = 0; G.pre && i0 < (size_t)n; i0 += first_cap * nfi) {
                const int nw = (int)std::min(first_cap * nfi, (size_t)n - i0), ni = (nw + nfi - 1) / nfi;
                KWS_LAUNCH_TRY("slide staging kernel", kws_launch_slide_stage_first(pcm, d_off, d_wbase, (int)A, (long long)(g0 + i0), nw, nfi, (int)G.S1, G.used, (long long)G.hop, (int)G.clip,
                                                                                    S.stage, S.wrap, st));
                if ((e = spectral_device(h, PF, S.stage, 0, ni, S.first + i0 * ncols, S.wrap, st, nfi * ncols))) return e;
            }
            KWS_LAUNCH_TRY("slide gather kernel", kws_launch_slide_gather(S.rows, S.first, d_wbase, d_sbase, d_ibase, (int)A, (long long)g0, n, (long long)G.phases, (long long)G.pitch, nfi,
                                                                          G.pre, G.nf, ncols, S.win, st));
        } else {
            // the windows as aligned clips (recordings as slots, windows as their items, one hop apart), then the handle's own plan
            for (size_t i0 = 0; i0 < (size_t)n; i0 += clip_cap) {
                const int nw = (int)std::min(clip_cap, (size_t)n - i0);
                KWS_LAUNCH_TRY("slide staging kernel", kws_launch_slide_stage(pcm, d_off, d_end, d_wbase, (int)A, (long long)(g0 + i0), nw, 1, (long long)G.hop, 0, (int)G.clip, 0, S.stage,
                                                                              nullptr, st));
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
    SlideGeom G;
    slide_geom(h, hop_samples, &G);
    *n_windows = G.windows(n_samples);
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
    SlideOwn own{ scores, features, KwsChunkCounts(h) };
    return kws_slide_run(h, pcm, offsets, lengths, R, hop_samples, flags, 1, slide_own_finish, &own, (hipStream_t)stream);
}

#pragma GCC visibility pop
}
