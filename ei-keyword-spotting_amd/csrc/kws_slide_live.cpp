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
// The finishing step is a callable (kws_slide_live_run): the above is what kws_slide_live_push_device passes; a bank passes cmvnw once + every
// member's network (kws_bank_windows.cpp).
// Reset touches no device memory: a stream's carry and rows are only read in the ranges its host counts say were written.
// Scratch, table upload, finishing step, fast counters, the session skeleton and the slide's geometry (SlideGeom): kws_windows.h.
#include "kws_internal.h"
#include "kws_windows.h"

int kws_launch_slide_live_stage_rows(const int16_t *pcm, const int16_t *carry, const long long *meta, int n_act, long long item0, int n_items,
                                     long long n_frames, int nfi, int S1, int used, int stride, long long hop, int clip, int pre, int16_t *stage,
                                     float *wrap, hipStream_t stream);
int kws_launch_slide_live_stage_clips(const int16_t *pcm, const int16_t *carry, const long long *meta, int n_act, long long win0, int n_win, long long hop,
                                      int clip, int16_t *stage, hipStream_t stream);
int kws_launch_slide_live_gather(const float *rows, const float *kept, const long long *meta, int n_act, long long win0, int n_win, long long hs, int run,
                                 int pre, int ncols, float *out, hipStream_t stream);
int kws_launch_slide_live_commit(const int16_t *pcm, const float *rows, const long long *meta, int n_act, long long hop, int cap, int run, int ncols,
                                 int16_t *carry, float *kept, hipStream_t stream);

// (KwsLiveSession, kws_windows.h: the handle, the streams' sample counts, carry [S][clip], kept [S][run][ncols] (shared path), the per-push scratch)
struct kws_slide_live : KwsLiveSession {
    std::vector<unsigned long long> &pc = m2;      // per stream: shared positions computed (shared path)
    SlideGeom G;                           // the slide's geometry at the session's hop
    size_t hs = 0;                         // hop / stride where the retained-row path serves the hop
    int path = KWS_SLIDE_DIRECT;

    unsigned long long positions(size_t W) const { return path == KWS_SLIDE_SHARED && W ? (unsigned long long)(W - 1) * hs + (unsigned long long)G.run : 0; }
};

// The finishing step of kws_slide_live_push_device itself: cmvnw + the handle's network in the handle's mode, chunk by chunk (h->mu held)
struct SlideLiveOwn {
    kws_slide_live *sl;
    float *scores, *features;
    KwsChunkCounts counts;
    bool started = false;
};
static EI_IMPULSE_ERROR slide_live_own_finish(void *ctx, float *win, size_t n, size_t g0, hipStream_t st)
{
    SlideLiveOwn &o = *(SlideLiveOwn *)ctx;
    kws_handle *h = o.sl->h;
    const size_t F = h->model.nn_input_frame_size, C = h->model.labels.size();
    EI_IMPULSE_ERROR e;
    if (!o.started) {
        // a push without a window: the fast counters describe it
        if (n == 0) return KwsChunkCounts::wanted(h) ? KwsChunkCounts::none(h, st) : EI_IMPULSE_OK;
        o.started = true;
        if ((e = o.counts.begin(o.sl->scratch.acc, n, st))) return e;
    }
    if (n == 0) return o.counts.end(st);                           // after the last chunk
    if ((e = kws_finish_window_chunk(h, win, n, o.scores + g0 * C, o.features ? o.features + g0 * F : nullptr, o.counts.fast, st))) return e;
    return o.counts.chunk(st);
}

// The push: argument checks, every count, the rows or clips of the completed windows, windows gathered in chunks through finish(), the
// commit of carry and retained rows, and the mirrors (kws_internal.h has the hook's contract).
EI_IMPULSE_ERROR kws_slide_live_run(kws_slide_live *sl, size_t n, const size_t *streams, const int16_t *pcm, const size_t *offsets, const size_t *lengths,
                                    const void *out, size_t *n_windows, size_t labels, int take_lock, int finish_idle, kws_slide_finish_fn finish, void *ctx,
                                    hipStream_t st)
{
    kws_handle *h = sl->h;
    const SlideGeom &G = sl->G;
    const bool shared = sl->path == KWS_SLIDE_SHARED;
    std::unique_lock<std::mutex> lk(h->mu, std::defer_lock);
    if (take_lock) lk.lock();
    // argument checks and every count of the push, before any state changes
    EI_IMPULSE_ERROR e = sl->check_push(n, streams, pcm, offsets, lengths, n_windows, (const float *)out);
    if (e) return e;
    // the entries with device work (A of them): windows, or new samples to carry
    std::vector<size_t> counts(n, 0);
    std::vector<long long> off, n0, len, sid, w0, pc0, np, rbase(1, 0), wbase(1, 0);
    for (size_t i = 0; i < n; ++i) {
        const size_t s = streams[i];
        if (!lengths[i]) continue;
        const size_t a0 = G.windows(sl->n[s]), a1 = G.windows(sl->n[s] + lengths[i]);
        counts[i] = a1 - a0;
        const unsigned long long p0 = sl->pc[s], p1 = sl->positions(a1);
        off.push_back((long long)offsets[i]);
        n0.push_back((long long)sl->n[s]);
        len.push_back((long long)lengths[i]);
        sid.push_back((long long)s);
        w0.push_back((long long)a0);
        pc0.push_back((long long)p0);
        np.push_back((long long)(p1 - p0));
        rbase.push_back(rbase.back() + (shared ? (long long)(p1 - p0) + (long long)(G.pre ? a1 - a0 : 0) : 0));
        wbase.push_back(wbase.back() + (long long)(a1 - a0));
    }
    const int A = (int)off.size();
    const size_t n_frames = (size_t)rbase.back(), n_win = (size_t)wbase.back();
    const Model &m = h->model;
    const size_t F = m.nn_input_frame_size, C = labels;
    const int ncols = G.ncols, nfi = G.nfi;
    if (n_win > (size_t)1 << 40 || n_win * C > (size_t)1 << 40) return fail(KWS_ERROR_BAD_ARGUMENT, "too many windows");
    for (size_t i = 0; i < n; ++i) n_windows[i] = counts[i];
    auto commit_mirrors = [&]() {
        for (size_t i = 0; i < n; ++i) {
            const size_t s = streams[i];
            sl->n[s] += lengths[i];
            sl->pc[s] = sl->positions(G.windows(sl->n[s]));
        }
    };
    if (A == 0 && !finish_idle) {
        commit_mirrors();
        return EI_IMPULSE_OK;
    }
    HIP_TRY(hipSetDevice(h->device));
    KwsWindowScratch &S = sl->scratch;
    // staged items: a rows item is nfi frames of S1 samples; a direct item is a window
    const size_t item_len = (size_t)nfi * G.S1, n_items = (n_frames + nfi - 1) / nfi;
    const size_t item_cap = kws_window_item_cap(item_len), clip_cap = kws_window_item_cap(G.clip), win_chunk = kws_window_chunk(F, n_win);
    const size_t stage_need = shared ? std::min(item_cap, std::max<size_t>(n_items, 1)) * item_len : std::min(clip_cap, win_chunk) * G.clip;
    const size_t wrap_need = shared ? std::min(item_cap, std::max<size_t>(n_items, 1)) : 1;
    if ((e = S.reserve(h, stage_need, wrap_need, win_chunk * F, std::max<size_t>(n_items * nfi * ncols, 1), 7 * (size_t)A + 2 * ((size_t)A + 1), win_chunk)))
        return e;
    ScratchUse use(h, st);
    if (n_win == 0) {
        if ((e = finish(ctx, nullptr, 0, 0, st))) return e;
        if (A == 0) {
            commit_mirrors();
            return EI_IMPULSE_OK;
        }
    }
    // per-entry tables (kws_slide_live_kernels.hip KwsSlideLiveMeta)
    if ((e = kws_upload_tables(S, { &off, &n0, &len, &sid, &w0, &pc0, &np, &rbase, &wbase }, st))) return e;
    if (shared && n_items) {
        // 1. the rows this push needs: nfi independent frames per item, S1 samples apart, each with its predecessor in the sample before it
        const KwsDspPlan PF = G.first_plan(h);
        for (size_t g0 = 0; g0 < n_items; g0 += item_cap) {
            const int c = (int)std::min(item_cap, n_items - g0);
            KWS_LAUNCH_TRY("slide live staging kernel", kws_launch_slide_live_stage_rows(pcm, sl->carry, S.meta, A, (long long)g0, c, (long long)n_frames, nfi, (int)G.S1, G.used, G.stride,
                                                                                         (long long)G.hop, (int)G.clip, G.pre, S.stage, S.wrap, st));
            if ((e = spectral_device(h, PF, S.stage, 0, c, S.rows + g0 * nfi * ncols, S.wrap, st, nfi * ncols))) return e;
        }
    }
    // 2. windows in chunks through the finishing step (cmvnw + the network)
    for (size_t g0 = 0; g0 < n_win; g0 += win_chunk) {
        const int c = (int)std::min(win_chunk, n_win - g0);
        if (shared) {
            KWS_LAUNCH_TRY("slide live gather kernel", kws_launch_slide_live_gather(S.rows, sl->kept, S.meta, A, (long long)g0, c, (long long)sl->hs, G.run, G.pre, ncols, S.win, st));
        } else {
            for (size_t i0 = 0; i0 < (size_t)c; i0 += clip_cap) {
                const int nw = (int)std::min(clip_cap, (size_t)c - i0);
                KWS_LAUNCH_TRY("slide live staging kernel", kws_launch_slide_live_stage_clips(pcm, sl->carry, S.meta, A, (long long)(g0 + i0), nw, (long long)G.hop, (int)G.clip, S.stage, st));
                if ((e = spectral_device(h, h->dsp, S.stage, 0, nw, S.win + i0 * F, nullptr, st, 0))) return e;
            }
        }
        if ((e = finish(ctx, S.win, (size_t)c, g0, st))) return e;
    }
    if (n_win && (e = finish(ctx, S.win, 0, n_win, st))) return e;
    // 3. the new carry and retained rows (after every read of the old ones above)
    KWS_LAUNCH_TRY("slide live commit kernel", kws_launch_slide_live_commit(pcm, S.rows, S.meta, A, (long long)G.hop, (int)G.clip, shared ? G.run : 0, ncols, sl->carry, sl->kept, st));
    commit_mirrors();
    return EI_IMPULSE_OK;
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
    kws_slide_live *sl = new kws_slide_live();
    sl->open(h, S);
    SlideGeom &G = sl->G;
    slide_geom(h, hop_samples, &G);
    // the retained-row path: the slide's phases == 1 and its "touching" case
    const bool served = G.phases == 1 && G.touching;
    if (flags == KWS_SLIDE_SHARED && !served) {
        delete sl;
        return fail(KWS_ERROR_BAD_ARGUMENT, "the retained-row path does not serve a hop of %zu samples", hop_samples);
    }
    sl->hs = served ? G.hg : 0;
    // the AUTO rule, the slide's by row count: the shared path where it computes fewer rows per window than the direct one
    sl->path = flags != KWS_SLIDE_AUTO ? flags : served && sl->hs + (size_t)G.pre < (size_t)G.nf ? KWS_SLIDE_SHARED : KWS_SLIDE_DIRECT;
    if (hipSetDevice(h->device) != hipSuccess) {
        delete sl;
        return fail(KWS_ERROR_HIP, "hipSetDevice failed");
    }
    const size_t carry_b = S * G.clip * sizeof(int16_t);
    const size_t kept_b = sl->path == KWS_SLIDE_SHARED ? S * (size_t)G.run * G.ncols * sizeof(float) : 0;
    bool ok = hipMalloc((void **)&sl->carry, carry_b) == hipSuccess && (!kept_b || hipMalloc((void **)&sl->kept, kept_b) == hipSuccess);
    // (nothing reads these before a push has written it; cleared so that no stale value can ever reach a result)
    ok = ok && hipMemset(sl->carry, 0, carry_b) == hipSuccess && (!kept_b || hipMemset(sl->kept, 0, kept_b) == hipSuccess);
    if (!ok) {
        sl->free_device();
        delete sl;
        return fail(KWS_ERROR_HIP, "slide live session allocation failed");
    }
    *out = sl;
    return EI_IMPULSE_OK;
}

void kws_slide_live_destroy(kws_slide_live *sl) { kws_session_destroy(sl); }

int kws_slide_live_path(const kws_slide_live *sl) { return sl ? sl->path : 0; }

EI_IMPULSE_ERROR kws_slide_live_reset(kws_slide_live *sl, const size_t *streams, size_t n)
{
    if (!sl) return fail(KWS_ERROR_BAD_ARGUMENT, "null argument");
    return sl->reset(streams, n);
}

EI_IMPULSE_ERROR kws_slide_live_window_count(const kws_slide_live *sl, size_t stream, size_t n_new, size_t *n_windows)
{
    if (!sl) return fail(KWS_ERROR_BAD_ARGUMENT, "null argument");
    return sl->window_count(stream, n_new, n_windows, [&](unsigned long long n0, unsigned long long n1) { return sl->G.windows(n1) - sl->G.windows(n0); });
}

EI_IMPULSE_ERROR kws_slide_live_push_device(kws_slide_live *sl, size_t n, const size_t *streams, const int16_t *pcm, const size_t *offsets,
                                            const size_t *lengths, float *scores, float *features, size_t *n_windows, void *stream)
{
    if (!sl) return fail(KWS_ERROR_BAD_ARGUMENT, "null argument");
    kws_handle *h = sl->h;
    std::lock_guard<std::mutex> lk(h->mu);
    SlideLiveOwn own{ sl, scores, features, KwsChunkCounts(h) };
    return kws_slide_live_run(sl, n, streams, pcm, offsets, lengths, scores, n_windows, h->model.labels.size(), 0, KwsChunkCounts::wanted(h) && h->d_flags,
                              slide_live_own_finish, &own, (hipStream_t)stream);
}

#pragma GCC visibility pop
}
