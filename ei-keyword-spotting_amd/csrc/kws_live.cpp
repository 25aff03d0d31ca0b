// kws_live.cpp -- live streams in continuous mode (kws_live_*; contract in include/kws/kws.h): audio of any length pushed to any subset of
// S streams, every window the pushed samples complete returned by the push, per-stream state kept in HBM between pushes.
//
// A stream is the recording scan (kws_scan.cpp) cut into pushes.  Its samples, numbered from its start, make slices k of `slice` samples;
// slice k >= 1 also reads its look-ahead sample k slice + slice + grow - 1, so it is FINISHED (its cepstral rows can be computed) once that
// sample has arrived, or when the stream is finished (past the end the sample is 0).  A push finishes the slices [k0, k1) of each entry and
// returns the windows that end in them: windows(k1) - windows(k0), the scan's window rule.  What a stream carries between pushes:
//   - its samples [k0 slice, n) (the next slices and their look-ahead: fewer than slice + grow), in a ring of slice + grow samples;
//   - its last min(rows, ring_rows - nf1) cepstral rows (what its next window reuses), in a ring of ring_rows - nf1 rows;
//   - the moving-average filter of each label (taps and running sum; the index is the window count mod taps).
// Host copies of each stream's sample and finished-slice counts give every count of a push before anything is launched.  A push launches:
//   1. kws_live_stage_kernel over its finished slices (slice-0 items, then slices k >= 1), each assembled from the carry and the chunk, and
//      the stream API's spectral launches (spectral_device) on them -- the scan's front end;
//   2. per chunk of windows: kws_live_gather_kernel (retained rows + this push's rows -> [chunk][F]), then cmvn_nn_device, or
//      cmvn_nn_fast_device in KWS_MODE_FAST, writing raw scores in place;
//   3. kws_live_commit_kernel: each continuing stream's new carry and retained rows;
//   4. kws_live_maf_kernel: the moving average per (entry, label), resumed from the stored filter.
// Steps 2 and 4 end in callables (kws_live_run: the finishing hook per chunk, the moving-average hook): what is written above is what
// kws_live_push_device passes; a bank passes cmvnw once + every member's network and one filter launch for all, on a session opened
// without filter state (kws_live_open; kws_bank_windows.cpp).
// Finish and reset touch no device memory: a stream with no window before a push starts from fresh state, and its carry and rows are only
// read in the ranges its host counts say were written.
// Scratch, table upload, finishing step, fast counters and the session skeleton (mirrors, push checks, reset, destroy): kws_windows.h.
#include "kws_internal.h"
#include "kws_windows.h"

#include "../../include/kws/ei_compat.h"

int kws_launch_live_stage(const int16_t *pcm, const int16_t *carry, const long long *meta, int n_act, long long item0, int n_items, int first, int slice,
                          int grow, int cap, int16_t *stage, float *wrap, hipStream_t stream);
int kws_launch_live_gather(const float *first_rows, const float *slot_rows, const float *kept, const long long *meta, int n_act, long long win0, int n_win,
                           int nf0, int nf1, int ring_rows, int keep, int k_full, int rows, int ncols, float *out, hipStream_t stream);
int kws_launch_live_commit(const int16_t *pcm, const float *first_rows, const float *slot_rows, const long long *meta, int n_act, int slice, int cap, int nf0,
                           int nf1, int keep, int ncols, int16_t *carry, float *kept, hipStream_t stream);
int kws_launch_live_maf(const float *raw, float *scores, const long long *meta, int n_act, int labels, int k_full, float *maf, hipStream_t stream);

static const int kLiveTaps = EI_CLASSIFIER_SLICES_PER_MODEL_WINDOW >> 1;

// (KwsLiveSession, kws_windows.h: the handle, the streams' sample counts, carry [S][cap], kept [S][max(keep, 1)][ncols], the per-push scratch)
struct kws_live : KwsLiveSession {
    std::vector<unsigned long long> &k = m2;       // per stream: finished slices
    size_t slice = 0;
    ScanLayout L;
    int cap = 0, keep = 0;                 // carry ring (samples), retained-row ring (rows)
    float *maf = nullptr;                  // state in HBM: [S][labels][taps + 1]

    // slices a stream of n1 samples has finished: slice 0 once complete, slice k >= 1 once its look-ahead sample has arrived; all complete ones at finish
    size_t finished(unsigned long long n1, bool fin) const
    {
        if (fin || n1 < slice) return (size_t)(n1 / slice);
        const unsigned long long g = (unsigned long long)L.grow;
        return std::max<size_t>(1, n1 >= g ? (size_t)((n1 - g) / slice) : 0);
    }
    void free_device()
    {
        if (maf) (void)hipFree(maf);
        maf = nullptr;
        KwsLiveSession::free_device();
    }
};

// The session of kws_live_create; with_maf == 0: without the moving-average state, which the caller keeps (a bank: one per member)
EI_IMPULSE_ERROR kws_live_open(kws_handle *h, size_t S, size_t slice_samples, int with_maf, kws_live **out)
{
    if (out) *out = nullptr;
    if (!h || !out || S == 0 || S > 0x3fffffff) return fail(KWS_ERROR_BAD_ARGUMENT, "bad argument");
    ScanLayout L;
    EI_IMPULSE_ERROR e = scan_layout(h, slice_samples, &L);
    if (e) return e;
    HIP_TRY(hipSetDevice(h->device));
    kws_live *lv = new kws_live();
    lv->open(h, S);
    lv->slice = slice_samples; lv->L = L;
    lv->cap = (int)slice_samples + L.grow;
    lv->keep = L.ring_rows - L.nf1;
    const size_t ncols = (size_t)h->dsp.n_cepstral, C = h->model.labels.size();
    const size_t carry_b = S * lv->cap * sizeof(int16_t), kept_b = S * std::max(lv->keep, 1) * ncols * sizeof(float);
    const size_t maf_b = with_maf ? S * C * (kLiveTaps + 1) * sizeof(float) : 0;
    bool ok = hipMalloc((void **)&lv->carry, carry_b) == hipSuccess && hipMalloc((void **)&lv->kept, kept_b) == hipSuccess &&
              (!maf_b || hipMalloc((void **)&lv->maf, maf_b) == hipSuccess);
    // (nothing reads these before a push has written it; cleared so that no stale value can ever reach a result)
    ok = ok && hipMemset(lv->carry, 0, carry_b) == hipSuccess && hipMemset(lv->kept, 0, kept_b) == hipSuccess &&
         (!maf_b || hipMemset(lv->maf, 0, maf_b) == hipSuccess);
    if (!ok) {
        lv->free_device();
        delete lv;
        return fail(KWS_ERROR_HIP, "live session allocation failed");
    }
    *out = lv;
    return EI_IMPULSE_OK;
}

// The finishing and moving-average steps of kws_live_push_device itself: cmvnw + the handle's network in the handle's mode, chunk by chunk,
// raw scores where the moving average reads them; then the filters resumed per (stream, label) (h->mu held)
struct LiveOwn {
    kws_live *lv;
    float *scores, *raw;
    KwsChunkCounts counts;
    bool started = false;
};
static EI_IMPULSE_ERROR live_own_finish(void *ctx, float *win, size_t n, size_t g0, hipStream_t st)
{
    LiveOwn &o = *(LiveOwn *)ctx;
    kws_handle *h = o.lv->h;
    EI_IMPULSE_ERROR e;
    if (!o.started) {
        // a push without a window: the fast counters describe it
        if (n == 0) return KwsChunkCounts::wanted(h) ? KwsChunkCounts::none(h, st) : EI_IMPULSE_OK;
        o.started = true;
        if ((e = o.counts.begin(o.lv->scratch.acc, n, st))) return e;
    }
    if (n == 0) return o.counts.end(st);                           // after the last chunk
    if ((e = kws_finish_window_chunk(h, win, n, o.raw + g0 * h->model.labels.size(), nullptr, o.counts.fast, st))) return e;
    return o.counts.chunk(st);
}
static EI_IMPULSE_ERROR live_own_maf(void *ctx, const long long *meta, int n_act, hipStream_t st)
{
    LiveOwn &o = *(LiveOwn *)ctx;
    KWS_LAUNCH_TRY("live moving-average kernel", kws_launch_live_maf(o.raw, o.scores, meta, n_act, (int)o.lv->h->model.labels.size(), (int)o.lv->L.k_full, o.lv->maf, st));
    return EI_IMPULSE_OK;
}

// The push: argument checks, every count, the front end of the finished slices, windows gathered in chunks through finish(), the commit of
// carry and retained rows, then maf() when the push has windows, and the mirrors (kws_internal.h has the hooks' contract).
EI_IMPULSE_ERROR kws_live_run(kws_live *lv, size_t n, const size_t *streams, const int16_t *pcm, const size_t *offsets, const size_t *lengths,
                              const int *finish_flags, const void *out, size_t *n_windows, size_t labels, int take_lock, int finish_idle,
                              kws_slide_finish_fn finish_fn, kws_window_maf_fn maf, void *ctx, hipStream_t st)
{
    kws_handle *h = lv->h;
    const ScanLayout &L = lv->L;
    const size_t slice = lv->slice;
    const int *finish = finish_flags;
    std::unique_lock<std::mutex> lk(h->mu, std::defer_lock);
    if (take_lock) lk.lock();
    // argument checks and every count of the push, before any state changes
    EI_IMPULSE_ERROR e = lv->check_push(n, streams, pcm, offsets, lengths, n_windows, (const float *)out);
    if (e) return e;
    // the entries with device work (A of them): windows, or a continuing stream's new samples
    std::vector<long long> off, n0, len, sid, k0, k1, fin, fbase(1, 0), ibase(1, 0), wbase(1, 0);
    for (size_t i = 0; i < n; ++i) {
        const size_t s = streams[i];
        const bool f = finish && finish[i];
        const size_t a0 = lv->k[s], a1 = lv->finished(lv->n[s] + lengths[i], f);
        n_windows[i] = L.windows(a1) - L.windows(a0);
        if (!n_windows[i] && (f || !lengths[i])) continue;
        off.push_back(lengths[i] ? (long long)offsets[i] : 0);
        n0.push_back((long long)lv->n[s]);
        len.push_back((long long)lengths[i]);
        sid.push_back((long long)s);
        k0.push_back((long long)a0);
        k1.push_back((long long)a1);
        fin.push_back(f ? 1 : 0);
        fbase.push_back(fbase.back() + (a0 == 0 && a1 > 0 ? 1 : 0));
        ibase.push_back(ibase.back() + (long long)(a1 > 1 ? a1 - std::max<size_t>(a0, 1) : 0));
        wbase.push_back(wbase.back() + (long long)n_windows[i]);
    }
    const int A = (int)off.size();
    const size_t n_first = (size_t)fbase.back(), n_slots = (size_t)ibase.back(), n_win = (size_t)wbase.back();
    const Model &m = h->model;
    const size_t F = m.nn_input_frame_size, C = labels;
    const int ncols = h->dsp.n_cepstral, rows = (int)(F / (size_t)ncols);
    if (n_win * C > (size_t)1 << 40) return fail(KWS_ERROR_BAD_ARGUMENT, "too many windows");
    auto commit_mirrors = [&]() {
        for (size_t i = 0; i < n; ++i) {
            const size_t s = streams[i];
            const bool f = finish && finish[i];
            if (f) { lv->n[s] = 0; lv->k[s] = 0; }
            else { lv->n[s] += lengths[i]; lv->k[s] = lv->finished(lv->n[s], false); }
        }
    };
    if (A == 0 && !finish_idle) {
        commit_mirrors();
        return EI_IMPULSE_OK;
    }
    HIP_TRY(hipSetDevice(h->device));
    KwsWindowScratch &S = lv->scratch;
    const size_t item_cap = kws_window_item_cap(slice), win_chunk = kws_window_chunk(F, n_win);
    const size_t first_floats = n_first * L.nf0 * ncols, rows_floats = std::max<size_t>(first_floats + n_slots * L.nf1 * ncols, 1);
    if ((e = S.reserve(h, item_cap * slice, item_cap, win_chunk * F, rows_floats, 7 * (size_t)A + 3 * ((size_t)A + 1), win_chunk))) return e;
    ScratchUse use(h, st);
    if (n_win == 0) {
        if ((e = finish_fn(ctx, nullptr, 0, 0, st))) return e;
        if (A == 0) {
            commit_mirrors();
            return EI_IMPULSE_OK;
        }
    }
    // per-entry tables (kws_live_kernels.hip KwsLiveMeta)
    if ((e = kws_upload_tables(S, { &off, &n0, &len, &sid, &k0, &k1, &fin, &fbase, &ibase, &wbase }, st))) return e;
    const int sl = (int)slice;
    float *first_rows = S.rows, *slot_rows = S.rows + first_floats;
    // 1. front end: the finished slices, assembled from carry and chunk, through the stream API's spectral launches
    KwsDspPlan P0 = h->dsp, P1 = h->dsp;
    P0.n_samples = P1.n_samples = sl;
    P0.n_frames = L.nf0;
    P1.n_frames = L.nf1;
    for (size_t g0 = 0; g0 < n_first; g0 += item_cap) {
        const int c = (int)std::min(item_cap, n_first - g0);
        KWS_LAUNCH_TRY("live staging kernel", kws_launch_live_stage(pcm, lv->carry, S.meta, A, (long long)g0, c, 1, sl, L.grow, lv->cap, S.stage, S.wrap, st));
        if ((e = spectral_device(h, P0, S.stage, 0, c, first_rows + g0 * L.nf0 * ncols, nullptr, st, L.nf0 * ncols))) return e;
    }
    for (size_t g0 = 0; g0 < n_slots; g0 += item_cap) {
        const int c = (int)std::min(item_cap, n_slots - g0);
        KWS_LAUNCH_TRY("live staging kernel", kws_launch_live_stage(pcm, lv->carry, S.meta, A, (long long)g0, c, 0, sl, L.grow, lv->cap, S.stage, S.wrap, st));
        if ((e = spectral_device(h, P1, S.stage, 0, c, slot_rows + g0 * L.nf1 * ncols, S.wrap, st, L.nf1 * ncols))) return e;
    }
    // 2. windows in chunks through the finishing step (the stream API's cmvnw + network); raw scores land where the moving average reads them
    for (size_t g0 = 0; g0 < n_win; g0 += win_chunk) {
        const int c = (int)std::min(win_chunk, n_win - g0);
        KWS_LAUNCH_TRY("live gather kernel", kws_launch_live_gather(first_rows, slot_rows, lv->kept, S.meta, A, (long long)g0, c, L.nf0, L.nf1, L.ring_rows, lv->keep, (int)L.k_full,
                                                                    rows, ncols, S.win, st));
        if ((e = finish_fn(ctx, S.win, (size_t)c, g0, st))) return e;
    }
    if (n_win && (e = finish_fn(ctx, S.win, 0, n_win, st))) return e;
    // 3. the continuing streams' carry and retained rows (after every read of the old ones above)
    KWS_LAUNCH_TRY("live commit kernel", kws_launch_live_commit(pcm, first_rows, slot_rows, S.meta, A, sl, lv->cap, L.nf0, L.nf1, lv->keep, ncols, lv->carry, lv->kept, st));
    // 4. the moving average, resumed per (stream, label)
    if (n_win && (e = maf(ctx, S.meta, A, st))) return e;
    commit_mirrors();
    return EI_IMPULSE_OK;
}

extern "C" {
#pragma GCC visibility push(default)

EI_IMPULSE_ERROR kws_live_create(kws_handle *h, size_t S, size_t slice_samples, kws_live **out) { return kws_live_open(h, S, slice_samples, 1, out); }

void kws_live_destroy(kws_live *lv) { kws_session_destroy(lv); }

EI_IMPULSE_ERROR kws_live_reset(kws_live *lv, const size_t *streams, size_t n)
{
    if (!lv) return fail(KWS_ERROR_BAD_ARGUMENT, "null argument");
    return lv->reset(streams, n);
}

EI_IMPULSE_ERROR kws_live_window_count(const kws_live *lv, size_t stream, size_t n_new, int finish, size_t *n_windows)
{
    if (!lv) return fail(KWS_ERROR_BAD_ARGUMENT, "null argument");
    return lv->window_count(stream, n_new, n_windows, [&](unsigned long long, unsigned long long n1) {
        return lv->L.windows(lv->finished(n1, finish != 0)) - lv->L.windows(lv->k[stream]);
    });
}

EI_IMPULSE_ERROR kws_live_push_device(kws_live *lv, size_t n, const size_t *streams, const int16_t *pcm, const size_t *offsets, const size_t *lengths,
                                      const int *finish, float *scores, float *raw_scores, size_t *n_windows, void *stream)
{
    if (!lv) return fail(KWS_ERROR_BAD_ARGUMENT, "null argument");
    kws_handle *h = lv->h;
    std::lock_guard<std::mutex> lk(h->mu);
    LiveOwn own{ lv, scores, raw_scores ? raw_scores : scores, KwsChunkCounts(h) };
    return kws_live_run(lv, n, streams, pcm, offsets, lengths, finish, scores, n_windows, h->model.labels.size(), 0, KwsChunkCounts::wanted(h) && h->d_flags,
                        live_own_finish, live_own_maf, &own, (hipStream_t)stream);
}

#pragma GCC visibility pop
}
