// kws_slide_live.cpp -- live streams of one-shot windows (kws_slide_live_*; contract in include/kws/kws.h): audio of any length pushed to any
// subset of S streams, every one-shot window (run_classifier() on samples [w hop, w hop + clip) of the stream) the pushed samples complete
// returned by the push, per-stream state kept in HBM between pushes.
//
// A stream is the slide (kws_slide.cpp) cut into pushes.  Window w is complete once sample w hop + clip - 1 has arrived: a stream of n samples
// has windows(n) = n < clip ? 0 : (n - clip) / hop + 1 of them, and a push returns the windows [windows(n0), windows(n0 + len)).  Nothing
// waits for a look-ahead sample, so there is no finish.  What a stream carries between pushes:
//   - its samples from the next incomplete window's start, windows(n) hop, up to n (fewer than clip; none where the hop skips past n), in a
//     ring of clip samples;
//   - shared path: its last frames - pre cepstral rows, in a ring of as many rows.  Frame f >= pre of window w is THE cepstral row of the
//     stream's position w hop / stride + f (kws_slide.cpp's argument at phases == 1); shared position j is the frame at sample (j + pre)
//     stride, window w reads the positions [w hs, w hs + run) (hs = hop / stride, run = frames - pre), and W windows have computed
//     positions(W) = (W - 1) hs + run of them.  hs <= run (the slide's "touching" case): the next window's first position is never older than
//     the ring's oldest.
// Host copies of each stream's sample and computed-position counts give every count of a push before anything is launched.  A push launches:
//   shared path:  1. kws_slide_live_stage_rows_kernel over the rows it needs and no earlier push has computed -- the new shared positions and
//                    frame 0 of every completed window, each an independent frame with its own predecessor sample, nfi to an item at the
//                    slide's frame-0 pitch -- and spectral_device on the items with the slide's plan variant PF;
//                 2. per chunk of windows: kws_slide_live_gather_kernel (retained rows + this push's rows -> [chunk][F]);
//   direct path:  per chunk, kws_slide_live_stage_clips_kernel (carry + chunk -> aligned clips) and the handle's own plan into [chunk][F];
//   both:         the finishing step per chunk (cmvn_nn_device, or cmvn_nn_fast_device and the count kernel in KWS_MODE_FAST), then
//                 kws_slide_live_commit_kernel: each entry's new carry and retained rows, after every read of the old ones.
// Reset touches no device memory: a stream's carry and rows are only read in the ranges its host counts say were written.
#include "kws_internal.h"

int kws_launch_slide_live_stage_rows(const int16_t *pcm, const int16_t *carry, const long long *meta, int n_act, long long item0, int n_items,
                                     long long n_frames, int nfi, int S1, int used, int stride, long long hop, int clip, int pre, int16_t *stage,
                                     float *wrap, hipStream_t stream);
int kws_launch_slide_live_stage_clips(const int16_t *pcm, const int16_t *carry, const long long *meta, int n_act, long long win0, int n_win, long long hop,
                                      int clip, int16_t *stage, hipStream_t stream);
int kws_launch_slide_live_gather(const float *rows, const float *kept, const long long *meta, int n_act, long long win0, int n_win, long long hs, int run,
                                 int pre, int ncols, float *out, hipStream_t stream);
int kws_launch_slide_live_commit(const int16_t *pcm, const float *rows, const long long *meta, int n_act, long long hop, int cap, int run, int ncols,
                                 int16_t *carry, float *kept, hipStream_t stream);
int kws_launch_scan_count(int *flags, int *flags2, int *acc, int finish, hipStream_t stream);      // kws_scan_kernels.hip

// bounded scratch of one push: the slide's bounds (include/kws/kws.h)
static const size_t kSlStageBytes = (size_t)32 << 20;
static const size_t kSlWindowBytes = (size_t)64 << 20;
static const size_t kSlMaxItems = 16384, kSlMaxWindows = 32768;
static const int kSlItemFrames = 48;                                     // frames per item, as the slide's
static const unsigned long long kSlMaxSamples = 1ull << 60;             // samples of one stream between starts (positions stay in long long)

struct kws_slide_live {
    kws_handle *h = nullptr;
    size_t S = 0, hop = 0, clip = 0;
    int nf = 0, stride = 0, ncols = 0, used = 0;
    int pre = 0, run = 0;                  // 1: pre-emphasis block, frame 0 is per window; shared rows per window: nf - pre
    size_t hs = 0;                         // hop / stride where the retained-row path serves the hop
    int path = KWS_SLIDE_DIRECT;
    int nfi = 0;                           // frames per staged item
    std::vector<unsigned long long> n;     // per stream: samples since its start
    std::vector<unsigned long long> pc;    // per stream: shared positions computed (shared path)
    // state in HBM
    int16_t *carry = nullptr;              // [S][clip]
    float *kept = nullptr;                 // [S][run][ncols] (shared path)
    // per-push scratch, grown on demand
    int16_t *stage = nullptr;
    float *wrap = nullptr, *win = nullptr, *rows = nullptr;
    long long *meta = nullptr;
    int *acc = nullptr;
    size_t stage_cap = 0, wrap_cap = 0, win_cap = 0, rows_cap = 0, meta_cap = 0, acc_cap = 0;

    size_t windows(unsigned long long n1) const { return n1 < clip ? 0 : (size_t)((n1 - clip) / hop) + 1; }
    unsigned long long positions(size_t W) const { return path == KWS_SLIDE_SHARED && W ? (unsigned long long)(W - 1) * hs + (unsigned long long)run : 0; }
};

static void slide_live_free(kws_slide_live *sl)
{
    for (void *p : { (void *)sl->carry, (void *)sl->kept, (void *)sl->stage, (void *)sl->wrap, (void *)sl->win, (void *)sl->rows, (void *)sl->meta,
                     (void *)sl->acc })
        if (p) (void)hipFree(p);
    delete sl;
}

extern "C" {
#pragma GCC visibility push(default)

EI_IMPULSE_ERROR kws_slide_live_create(kws_handle *h, size_t S, size_t hop_samples, int flags, kws_slide_live **out)
{
    if (out) *out = nullptr;
    if (!h || !out || S == 0 || S > 0x3fffffff) return fail(KWS_ERROR_BAD_ARGUMENT, "bad argument");
    size_t w = 0;
    EI_IMPULSE_ERROR e = kws_slide_window_count(h, 0, hop_samples, &w);           // the slide's limits on a hop
    if (e) return e;
    if (flags != KWS_SLIDE_AUTO && flags != KWS_SLIDE_DIRECT && flags != KWS_SLIDE_SHARED) return fail(KWS_ERROR_BAD_ARGUMENT, "unknown flags %d", flags);
    const KwsDspPlan &P = h->dsp;
    kws_slide_live *sl = new kws_slide_live();
    sl->h = h; sl->S = S; sl->hop = hop_samples;
    sl->clip = h->model.raw_sample_count;
    sl->nf = P.n_frames; sl->stride = P.frame_stride; sl->ncols = P.n_cepstral;
    sl->used = std::min(P.frame_len, P.fft_len);
    sl->pre = h->model.dsp.block == DSP_BLOCK_MFE ? 0 : 1;
    sl->run = sl->nf - sl->pre;
    sl->nfi = std::max(1, std::min(kSlItemFrames, sl->nf));
    // the retained-row path: the slide's phases == 1 and its "touching" case
    const bool served = sl->stride > 0 && sl->run > 0 && hop_samples % (size_t)sl->stride == 0 && hop_samples / (size_t)sl->stride <= (size_t)sl->run;
    if (flags == KWS_SLIDE_SHARED && !served) {
        delete sl;
        return fail(KWS_ERROR_BAD_ARGUMENT, "the retained-row path does not serve a hop of %zu samples", hop_samples);
    }
    sl->hs = served ? hop_samples / (size_t)sl->stride : 0;
    // the AUTO rule, the slide's by row count: the shared path where it computes fewer rows per window than the direct one
    sl->path = flags != KWS_SLIDE_AUTO ? flags : served && sl->hs + (size_t)sl->pre < (size_t)sl->nf ? KWS_SLIDE_SHARED : KWS_SLIDE_DIRECT;
    sl->n.assign(S, 0);
    sl->pc.assign(S, 0);
    if (hipSetDevice(h->device) != hipSuccess) {
        delete sl;
        return fail(KWS_ERROR_HIP, "hipSetDevice failed");
    }
    const size_t carry_b = S * sl->clip * sizeof(int16_t);
    const size_t kept_b = sl->path == KWS_SLIDE_SHARED ? S * (size_t)sl->run * sl->ncols * sizeof(float) : 0;
    bool ok = hipMalloc((void **)&sl->carry, carry_b) == hipSuccess && (!kept_b || hipMalloc((void **)&sl->kept, kept_b) == hipSuccess);
    // (nothing reads these before a push has written it; cleared so that no stale value can ever reach a result)
    ok = ok && hipMemset(sl->carry, 0, carry_b) == hipSuccess && (!kept_b || hipMemset(sl->kept, 0, kept_b) == hipSuccess);
    if (!ok) {
        slide_live_free(sl);
        return fail(KWS_ERROR_HIP, "slide live session allocation failed");
    }
    *out = sl;
    return EI_IMPULSE_OK;
}

void kws_slide_live_destroy(kws_slide_live *sl)
{
    if (!sl) return;
    kws_handle *h = sl->h;
    std::lock_guard<std::mutex> lk(h->mu);
    (void)hipSetDevice(h->device);
    // every push brackets its work with ScratchUse: the handle's event marks the end of the latest call, this session's last push included
    if (h->scratch_used && h->scratch_ev) (void)hipEventSynchronize(h->scratch_ev);
    slide_live_free(sl);
}

int kws_slide_live_path(const kws_slide_live *sl) { return sl ? sl->path : 0; }

EI_IMPULSE_ERROR kws_slide_live_reset(kws_slide_live *sl, const size_t *streams, size_t n)
{
    if (!sl || (n > 0 && !streams)) return fail(KWS_ERROR_BAD_ARGUMENT, "null argument");
    std::lock_guard<std::mutex> lk(sl->h->mu);
    if (!streams) {
        std::fill(sl->n.begin(), sl->n.end(), 0);
        std::fill(sl->pc.begin(), sl->pc.end(), 0);
        return EI_IMPULSE_OK;
    }
    for (size_t i = 0; i < n; ++i)
        if (streams[i] >= sl->S) return fail(KWS_ERROR_BAD_ARGUMENT, "stream %zu of %zu", streams[i], sl->S);
    for (size_t i = 0; i < n; ++i) sl->n[streams[i]] = sl->pc[streams[i]] = 0;
    return EI_IMPULSE_OK;
}

EI_IMPULSE_ERROR kws_slide_live_window_count(const kws_slide_live *sl, size_t stream, size_t n_new, size_t *n_windows)
{
    if (!sl || !n_windows) return fail(KWS_ERROR_BAD_ARGUMENT, "null argument");
    *n_windows = 0;
    if (stream >= sl->S) return fail(KWS_ERROR_BAD_ARGUMENT, "stream %zu of %zu", stream, sl->S);
    std::lock_guard<std::mutex> lk(sl->h->mu);
    const unsigned long long n0 = sl->n[stream];
    if (n_new > kSlMaxSamples - n0) return fail(KWS_ERROR_BAD_ARGUMENT, "stream %zu: too many samples", stream);
    *n_windows = sl->windows(n0 + n_new) - sl->windows(n0);
    return EI_IMPULSE_OK;
}

EI_IMPULSE_ERROR kws_slide_live_push_device(kws_slide_live *sl, size_t n, const size_t *streams, const int16_t *pcm, const size_t *offsets,
                                            const size_t *lengths, float *scores, float *features, size_t *n_windows, void *stream)
{
    if (!sl) return fail(KWS_ERROR_BAD_ARGUMENT, "null argument");
    if (n > 0 && (!streams || !lengths || !n_windows || !scores)) return fail(KWS_ERROR_BAD_ARGUMENT, "null argument");
    if (n > sl->S) return fail(KWS_ERROR_BAD_ARGUMENT, "%zu entries for %zu streams", n, sl->S);
    kws_handle *h = sl->h;
    const bool shared = sl->path == KWS_SLIDE_SHARED;
    std::lock_guard<std::mutex> lk(h->mu);
    // argument checks and every count of the push, before any state changes
    std::vector<char> named(sl->S, 0);
    bool any_samples = false;
    for (size_t i = 0; i < n; ++i) {
        const size_t s = streams[i];
        if (s >= sl->S) return fail(KWS_ERROR_BAD_ARGUMENT, "entry %zu: stream %zu of %zu", i, s, sl->S);
        if (named[s]) return fail(KWS_ERROR_BAD_ARGUMENT, "entry %zu: stream %zu named twice", i, s);
        named[s] = 1;
        if (lengths[i] > kSlMaxSamples - sl->n[s]) return fail(KWS_ERROR_BAD_ARGUMENT, "entry %zu: too many samples", i);
        any_samples = any_samples || lengths[i] > 0;
    }
    if (any_samples && (!pcm || !offsets)) return fail(KWS_ERROR_BAD_ARGUMENT, "null argument");
    // the entries with device work (A of them): windows, or new samples to carry
    std::vector<size_t> counts(n, 0);
    std::vector<long long> off, n0, len, sid, w0, pc0, np, rbase(1, 0), wbase(1, 0);
    for (size_t i = 0; i < n; ++i) {
        const size_t s = streams[i];
        if (!lengths[i]) continue;
        const size_t a0 = sl->windows(sl->n[s]), a1 = sl->windows(sl->n[s] + lengths[i]);
        counts[i] = a1 - a0;
        const unsigned long long p0 = sl->pc[s], p1 = sl->positions(a1);
        off.push_back((long long)offsets[i]);
        n0.push_back((long long)sl->n[s]);
        len.push_back((long long)lengths[i]);
        sid.push_back((long long)s);
        w0.push_back((long long)a0);
        pc0.push_back((long long)p0);
        np.push_back((long long)(p1 - p0));
        rbase.push_back(rbase.back() + (shared ? (long long)(p1 - p0) + (long long)(sl->pre ? a1 - a0 : 0) : 0));
        wbase.push_back(wbase.back() + (long long)(a1 - a0));
    }
    const int A = (int)off.size();
    const size_t n_frames = (size_t)rbase.back(), n_win = (size_t)wbase.back();
    const Model &m = h->model;
    const size_t F = m.nn_input_frame_size, C = m.labels.size();
    const int ncols = sl->ncols, nfi = sl->nfi;
    if (n_win > (size_t)1 << 40 || n_win * C > (size_t)1 << 40) return fail(KWS_ERROR_BAD_ARGUMENT, "too many windows");
    for (size_t i = 0; i < n; ++i) n_windows[i] = counts[i];
    const bool fast = h->mode == KWS_MODE_FAST && h->fast_plain_ok;
    const bool count = fast && m.dsp.block != DSP_BLOCK_MFE;          // the MFE block's fast form is its exact one: no guard, no counts
    auto commit_mirrors = [&]() {
        for (size_t i = 0; i < n; ++i) {
            const size_t s = streams[i];
            sl->n[s] += lengths[i];
            sl->pc[s] = sl->positions(sl->windows(sl->n[s]));
        }
    };
    if (A == 0 && !(count && h->d_flags)) {
        commit_mirrors();
        return EI_IMPULSE_OK;
    }
    HIP_TRY(hipSetDevice(h->device));
    hipStream_t st = (hipStream_t)stream;
    EI_IMPULSE_ERROR e;
    // staged items: a rows item is nfi frames of S1 samples; a direct item is a window
    const size_t S1 = ((size_t)sl->used + 1 + 7) & ~(size_t)7, item_len = (size_t)nfi * S1;
    const size_t n_items = (n_frames + nfi - 1) / nfi;
    const size_t item_cap = std::max<size_t>(1, std::min(kSlMaxItems, kSlStageBytes / (item_len * sizeof(int16_t))));
    const size_t clip_cap = std::max<size_t>(1, std::min(kSlMaxItems, kSlStageBytes / (sl->clip * sizeof(int16_t))));
    const size_t win_chunk = std::min(std::max<size_t>(1, std::min(kSlMaxWindows, kSlWindowBytes / (F * sizeof(float)))), std::max<size_t>(n_win, 1));
    const size_t stage_need = shared ? std::min(item_cap, std::max<size_t>(n_items, 1)) * item_len : std::min(clip_cap, win_chunk) * sl->clip;
    const size_t wrap_need = shared ? std::min(item_cap, std::max<size_t>(n_items, 1)) : 1;
    const size_t meta_n = 7 * (size_t)A + 2 * ((size_t)A + 1);
    if ((e = grow_buffer(&sl->stage, &sl->stage_cap, stage_need)) || (e = grow_buffer(&sl->wrap, &sl->wrap_cap, wrap_need)) ||
        (e = grow_buffer(&sl->win, &sl->win_cap, win_chunk * F)) || (e = grow_buffer(&sl->rows, &sl->rows_cap, std::max<size_t>(n_items * nfi * ncols, 1))) ||
        (e = grow_buffer(&sl->meta, &sl->meta_cap, meta_n)) || (e = grow_buffer(&sl->acc, &sl->acc_cap, 1)) || (e = ensure_scratch(h, win_chunk)))
        return e;
    ScratchUse use(h, st);
    if (count && n_win == 0) {
        // kws_fast_fallback_count / kws_fast_exact_count describe the last push: none of its windows was handed back
        HIP_TRY(hipMemsetAsync(h->d_flags, 0, sizeof(int), st));
        HIP_TRY(hipMemsetAsync(h->d_flags2, 0, sizeof(int), st));
        if (A == 0) {
            commit_mirrors();
            return EI_IMPULSE_OK;
        }
    }
    // per-entry tables (kws_slide_live_kernels.hip KwsSlideLiveMeta).  The host copy is complete before the call goes on
    std::vector<long long> meta;
    meta.reserve(meta_n);
    for (const std::vector<long long> *v : { &off, &n0, &len, &sid, &w0, &pc0, &np, &rbase, &wbase }) meta.insert(meta.end(), v->begin(), v->end());
    HIP_TRY(hipMemcpyAsync(sl->meta, meta.data(), meta.size() * sizeof(long long), hipMemcpyHostToDevice, st));
    HIP_TRY(hipStreamSynchronize(st));
    int rc = 0;
    if (shared && n_items) {
        // 1. the rows this push needs: nfi independent frames per item, S1 samples apart, each with its predecessor in the sample before it
        KwsDspPlan PF = h->dsp;
        PF.frame_stride = (int)S1;
        PF.n_samples = (int)item_len;
        PF.n_frames = nfi;
        PF.wrap_index = PF.n_samples - 1;
        for (size_t g0 = 0; g0 < n_items; g0 += item_cap) {
            const int c = (int)std::min(item_cap, n_items - g0);
            rc = kws_launch_slide_live_stage_rows(pcm, sl->carry, sl->meta, A, (long long)g0, c, (long long)n_frames, nfi, (int)S1, sl->used, sl->stride,
                                                  (long long)sl->hop, (int)sl->clip, sl->pre, sl->stage, sl->wrap, st);
            if (rc) return fail(KWS_ERROR_HIP, "slide live staging kernel launch failed: %s", hipGetErrorString((hipError_t)rc));
            if ((e = spectral_device(h, PF, sl->stage, 0, c, sl->rows + g0 * nfi * ncols, sl->wrap, st, nfi * ncols))) return e;
        }
    }
    // 2. windows in chunks through the finishing step (cmvnw + the network)
    if (count && n_win) HIP_TRY(hipMemsetAsync(sl->acc, 0, sizeof(int), st));
    for (size_t g0 = 0; g0 < n_win; g0 += win_chunk) {
        const int c = (int)std::min(win_chunk, n_win - g0);
        if (shared) {
            rc = kws_launch_slide_live_gather(sl->rows, sl->kept, sl->meta, A, (long long)g0, c, (long long)sl->hs, sl->run, sl->pre, ncols, sl->win, st);
            if (rc) return fail(KWS_ERROR_HIP, "slide live gather kernel launch failed: %s", hipGetErrorString((hipError_t)rc));
        } else {
            for (size_t i0 = 0; i0 < (size_t)c; i0 += clip_cap) {
                const int nw = (int)std::min(clip_cap, (size_t)c - i0);
                rc = kws_launch_slide_live_stage_clips(pcm, sl->carry, sl->meta, A, (long long)(g0 + i0), nw, (long long)sl->hop, (int)sl->clip, sl->stage, st);
                if (rc) return fail(KWS_ERROR_HIP, "slide live staging kernel launch failed: %s", hipGetErrorString((hipError_t)rc));
                if ((e = spectral_device(h, h->dsp, sl->stage, 0, nw, sl->win + i0 * F, nullptr, st, 0))) return e;
            }
        }
        if ((e = kws_finish_window_chunk(h, sl->win, (size_t)c, scores + g0 * C, features ? features + g0 * F : nullptr, fast, st))) return e;
        if (count && (rc = kws_launch_scan_count(h->d_flags, h->d_flags2, sl->acc, 0, st)))
            return fail(KWS_ERROR_HIP, "slide live count kernel launch failed: %s", hipGetErrorString((hipError_t)rc));
    }
    if (count && n_win && (rc = kws_launch_scan_count(h->d_flags, h->d_flags2, sl->acc, 1, st)))
        return fail(KWS_ERROR_HIP, "slide live count kernel launch failed: %s", hipGetErrorString((hipError_t)rc));
    // 3. the new carry and retained rows (after every read of the old ones above)
    rc = kws_launch_slide_live_commit(pcm, sl->rows, sl->meta, A, (long long)sl->hop, (int)sl->clip, shared ? sl->run : 0, ncols, sl->carry, sl->kept, st);
    if (rc) return fail(KWS_ERROR_HIP, "slide live commit kernel launch failed: %s", hipGetErrorString((hipError_t)rc));
    commit_mirrors();
    return EI_IMPULSE_OK;
}

#pragma GCC visibility pop
}
