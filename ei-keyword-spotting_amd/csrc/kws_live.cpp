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
// Finish and reset touch no device memory: a stream with no window before a push starts from fresh state, and its carry and rows are only
// read in the ranges its host counts say were written.
#include "kws_internal.h"

#include "../../include/kws/ei_compat.h"

int kws_launch_live_stage(const int16_t *pcm, const int16_t *carry, const long long *meta, int n_act, long long item0, int n_items, int first, int slice,
                          int grow, int cap, int16_t *stage, float *wrap, hipStream_t stream);
int kws_launch_live_gather(const float *first_rows, const float *slot_rows, const float *kept, const long long *meta, int n_act, long long win0, int n_win,
                           int nf0, int nf1, int ring_rows, int keep, int k_full, int rows, int ncols, float *out, hipStream_t stream);
int kws_launch_live_commit(const int16_t *pcm, const float *first_rows, const float *slot_rows, const long long *meta, int n_act, int slice, int cap, int nf0,
                           int nf1, int keep, int ncols, int16_t *carry, float *kept, hipStream_t stream);
int kws_launch_live_maf(const float *raw, float *scores, const long long *meta, int n_act, int labels, int k_full, float *maf, hipStream_t stream);
int kws_launch_scan_count(int *flags, int *flags2, int *acc, int finish, hipStream_t stream);      // kws_scan_kernels.hip

static const int kLiveTaps = EI_CLASSIFIER_SLICES_PER_MODEL_WINDOW >> 1;
// bounded scratch of one push: the scan's bounds (include/kws/kws.h)
static const size_t kLiveStageBytes = (size_t)32 << 20;
static const size_t kLiveWindowBytes = (size_t)64 << 20;
static const size_t kLiveMaxItems = 16384, kLiveMaxWindows = 32768;
static const unsigned long long kLiveMaxSamples = 1ull << 60;           // samples of one stream between starts (positions stay in long long)

struct kws_live {
    kws_handle *h = nullptr;
    size_t S = 0, slice = 0;
    ScanLayout L;
    int cap = 0, keep = 0;                 // carry ring (samples), retained-row ring (rows)
    std::vector<unsigned long long> n;     // per stream: samples since its start
    std::vector<unsigned long long> k;     // per stream: finished slices
    // state in HBM
    int16_t *carry = nullptr;              // [S][cap]
    float *kept = nullptr;                 // [S][max(keep, 1)][ncols]
    float *maf = nullptr;                  // [S][labels][taps + 1]
    // per-push scratch, grown on demand
    int16_t *stage = nullptr;
    float *wrap = nullptr, *win = nullptr, *rows = nullptr;
    long long *meta = nullptr;
    int *acc = nullptr;
    size_t stage_cap = 0, wrap_cap = 0, win_cap = 0, rows_cap = 0, meta_cap = 0, acc_cap = 0;

    // slices a stream of n1 samples has finished: slice 0 once complete, slice k >= 1 once its look-ahead sample has arrived; all complete ones at finish
    size_t finished(unsigned long long n1, bool fin) const
    {
        if (fin || n1 < slice) return (size_t)(n1 / slice);
        const unsigned long long g = (unsigned long long)L.grow;
        return std::max<size_t>(1, n1 >= g ? (size_t)((n1 - g) / slice) : 0);
    }
};

static void live_free(kws_live *lv)
{
    for (void *p : { (void *)lv->carry, (void *)lv->kept, (void *)lv->maf, (void *)lv->stage, (void *)lv->wrap, (void *)lv->win, (void *)lv->rows,
                     (void *)lv->meta, (void *)lv->acc })
        if (p) (void)hipFree(p);
    delete lv;
}

extern "C" {
#pragma GCC visibility push(default)

EI_IMPULSE_ERROR kws_live_create(kws_handle *h, size_t S, size_t slice_samples, kws_live **out)
{
    if (out) *out = nullptr;
    if (!h || !out || S == 0 || S > 0x3fffffff) return fail(KWS_ERROR_BAD_ARGUMENT, "bad argument");
    ScanLayout L;
    EI_IMPULSE_ERROR e = scan_layout(h, slice_samples, &L);
    if (e) return e;
    HIP_TRY(hipSetDevice(h->device));
    kws_live *lv = new kws_live();
    lv->h = h; lv->S = S; lv->slice = slice_samples; lv->L = L;
    lv->cap = (int)slice_samples + L.grow;
    lv->keep = L.ring_rows - L.nf1;
    lv->n.assign(S, 0);
    lv->k.assign(S, 0);
    const size_t ncols = (size_t)h->dsp.n_cepstral, C = h->model.labels.size();
    const size_t carry_b = S * lv->cap * sizeof(int16_t), kept_b = S * std::max(lv->keep, 1) * ncols * sizeof(float);
    const size_t maf_b = S * C * (kLiveTaps + 1) * sizeof(float);
    bool ok = hipMalloc((void **)&lv->carry, carry_b) == hipSuccess && hipMalloc((void **)&lv->kept, kept_b) == hipSuccess &&
              hipMalloc((void **)&lv->maf, maf_b) == hipSuccess;
    // (nothing reads these before a push has written it; cleared so that no stale value can ever reach a result)
    ok = ok && hipMemset(lv->carry, 0, carry_b) == hipSuccess && hipMemset(lv->kept, 0, kept_b) == hipSuccess && hipMemset(lv->maf, 0, maf_b) == hipSuccess;
    if (!ok) {
        live_free(lv);
        return fail(KWS_ERROR_HIP, "live session allocation failed");
    }
    *out = lv;
    return EI_IMPULSE_OK;
}

void kws_live_destroy(kws_live *lv)
{
    if (!lv) return;
    kws_handle *h = lv->h;
    {
        std::lock_guard<std::mutex> lk(h->mu);
        (void)hipSetDevice(h->device);
        // every push brackets its work with ScratchUse: the handle's event marks the end of the latest call, this session's last push included
        if (h->scratch_used && h->scratch_ev) (void)hipEventSynchronize(h->scratch_ev);
        live_free(lv);
    }
}

EI_IMPULSE_ERROR kws_live_reset(kws_live *lv, const size_t *streams, size_t n)
{
    if (!lv || (n > 0 && !streams)) return fail(KWS_ERROR_BAD_ARGUMENT, "null argument");
    std::lock_guard<std::mutex> lk(lv->h->mu);
    if (!streams) {
        std::fill(lv->n.begin(), lv->n.end(), 0);
        std::fill(lv->k.begin(), lv->k.end(), 0);
        return EI_IMPULSE_OK;
    }
    for (size_t i = 0; i < n; ++i)
        if (streams[i] >= lv->S) return fail(KWS_ERROR_BAD_ARGUMENT, "stream %zu of %zu", streams[i], lv->S);
    for (size_t i = 0; i < n; ++i) lv->n[streams[i]] = lv->k[streams[i]] = 0;
    return EI_IMPULSE_OK;
}

EI_IMPULSE_ERROR kws_live_window_count(const kws_live *lv, size_t stream, size_t n_new, int finish, size_t *n_windows)
{
    if (!lv || !n_windows) return fail(KWS_ERROR_BAD_ARGUMENT, "null argument");
    *n_windows = 0;
    if (stream >= lv->S) return fail(KWS_ERROR_BAD_ARGUMENT, "stream %zu of %zu", stream, lv->S);
    std::lock_guard<std::mutex> lk(lv->h->mu);
    const unsigned long long n0 = lv->n[stream];
    if (n_new > kLiveMaxSamples - n0) return fail(KWS_ERROR_BAD_ARGUMENT, "stream %zu: too many samples", stream);
    *n_windows = lv->L.windows(lv->finished(n0 + n_new, finish != 0)) - lv->L.windows(lv->k[stream]);
    return EI_IMPULSE_OK;
}

EI_IMPULSE_ERROR kws_live_push_device(kws_live *lv, size_t n, const size_t *streams, const int16_t *pcm, const size_t *offsets, const size_t *lengths,
                                      const int *finish, float *scores, float *raw_scores, size_t *n_windows, void *stream)
{
    if (!lv) return fail(KWS_ERROR_BAD_ARGUMENT, "null argument");
    if (n > 0 && (!streams || !lengths || !n_windows || !scores)) return fail(KWS_ERROR_BAD_ARGUMENT, "null argument");
    if (n > lv->S) return fail(KWS_ERROR_BAD_ARGUMENT, "%zu entries for %zu streams", n, lv->S);
    kws_handle *h = lv->h;
    const ScanLayout &L = lv->L;
    const size_t slice = lv->slice;
    std::lock_guard<std::mutex> lk(h->mu);
    // argument checks and every count of the push, before any state changes
    std::vector<char> named(lv->S, 0);
    bool any_samples = false;
    for (size_t i = 0; i < n; ++i) {
        const size_t s = streams[i];
        if (s >= lv->S) return fail(KWS_ERROR_BAD_ARGUMENT, "entry %zu: stream %zu of %zu", i, s, lv->S);
        if (named[s]) return fail(KWS_ERROR_BAD_ARGUMENT, "entry %zu: stream %zu named twice", i, s);
        named[s] = 1;
        if (lengths[i] > kLiveMaxSamples - lv->n[s]) return fail(KWS_ERROR_BAD_ARGUMENT, "entry %zu: too many samples", i);
        any_samples = any_samples || lengths[i] > 0;
    }
    if (any_samples && (!pcm || !offsets)) return fail(KWS_ERROR_BAD_ARGUMENT, "null argument");
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
    const size_t F = m.nn_input_frame_size, C = m.labels.size();
    const int ncols = h->dsp.n_cepstral, rows = (int)(F / (size_t)ncols);
    if (n_win * C > (size_t)1 << 40) return fail(KWS_ERROR_BAD_ARGUMENT, "too many windows");
    const bool fast = h->mode == KWS_MODE_FAST && h->fast_plain_ok;
    const bool count = fast && m.dsp.block != DSP_BLOCK_MFE;          // the MFE block's fast form is its exact one: no guard, no counts
    auto commit_mirrors = [&]() {
        for (size_t i = 0; i < n; ++i) {
            const size_t s = streams[i];
            const bool f = finish && finish[i];
            if (f) { lv->n[s] = 0; lv->k[s] = 0; }
            else { lv->n[s] += lengths[i]; lv->k[s] = lv->finished(lv->n[s], false); }
        }
    };
    if (A == 0 && !(count && h->d_flags)) {
        commit_mirrors();
        return EI_IMPULSE_OK;
    }
    HIP_TRY(hipSetDevice(h->device));
    hipStream_t st = (hipStream_t)stream;
    EI_IMPULSE_ERROR e;
    const size_t item_cap = std::max<size_t>(1, std::min(kLiveMaxItems, kLiveStageBytes / (slice * sizeof(int16_t))));
    const size_t win_chunk = std::min(std::max<size_t>(1, std::min(kLiveMaxWindows, kLiveWindowBytes / (F * sizeof(float)))), std::max<size_t>(n_win, 1));
    const size_t first_floats = n_first * L.nf0 * ncols, rows_floats = std::max<size_t>(first_floats + n_slots * L.nf1 * ncols, 1);
    const size_t meta_n = 7 * (size_t)A + 3 * ((size_t)A + 1);
    if ((e = grow_buffer(&lv->stage, &lv->stage_cap, item_cap * slice)) || (e = grow_buffer(&lv->wrap, &lv->wrap_cap, item_cap)) ||
        (e = grow_buffer(&lv->win, &lv->win_cap, win_chunk * F)) || (e = grow_buffer(&lv->rows, &lv->rows_cap, rows_floats)) ||
        (e = grow_buffer(&lv->meta, &lv->meta_cap, meta_n)) || (e = grow_buffer(&lv->acc, &lv->acc_cap, 1)) || (e = ensure_scratch(h, win_chunk)))
        return e;
    // pushes write no logits tap (out of the tap's [B][labels] shape): the tap is set aside for the call
    struct TapAside {
        kws_handle *h; float *t;
        ~TapAside() { h->tap_logits = t; }
    } tap_aside{ h, h->tap_logits };
    h->tap_logits = nullptr;
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
    // per-entry tables (kws_live_kernels.hip KwsLiveMeta).  The host copy is complete before the call goes on
    std::vector<long long> meta;
    meta.reserve(meta_n);
    for (const std::vector<long long> *v : { &off, &n0, &len, &sid, &k0, &k1, &fin, &fbase, &ibase, &wbase }) meta.insert(meta.end(), v->begin(), v->end());
    HIP_TRY(hipMemcpyAsync(lv->meta, meta.data(), meta.size() * sizeof(long long), hipMemcpyHostToDevice, st));
    HIP_TRY(hipStreamSynchronize(st));
    const int sl = (int)slice;
    float *first_rows = lv->rows, *slot_rows = lv->rows + first_floats;
    // 1. front end: the finished slices, assembled from carry and chunk, through the stream API's spectral launches
    KwsDspPlan P0 = h->dsp, P1 = h->dsp;
    P0.n_samples = P1.n_samples = sl;
    P0.n_frames = L.nf0;
    P1.n_frames = L.nf1;
    for (size_t g0 = 0; g0 < n_first; g0 += item_cap) {
        const int c = (int)std::min(item_cap, n_first - g0);
        int rc = kws_launch_live_stage(pcm, lv->carry, lv->meta, A, (long long)g0, c, 1, sl, L.grow, lv->cap, lv->stage, lv->wrap, st);
        if (rc) return fail(KWS_ERROR_HIP, "live staging kernel launch failed: %s", hipGetErrorString((hipError_t)rc));
        if ((e = spectral_device(h, P0, lv->stage, 0, c, first_rows + g0 * L.nf0 * ncols, nullptr, st, L.nf0 * ncols))) return e;
    }
    for (size_t g0 = 0; g0 < n_slots; g0 += item_cap) {
        const int c = (int)std::min(item_cap, n_slots - g0);
        int rc = kws_launch_live_stage(pcm, lv->carry, lv->meta, A, (long long)g0, c, 0, sl, L.grow, lv->cap, lv->stage, lv->wrap, st);
        if (rc) return fail(KWS_ERROR_HIP, "live staging kernel launch failed: %s", hipGetErrorString((hipError_t)rc));
        if ((e = spectral_device(h, P1, lv->stage, 0, c, slot_rows + g0 * L.nf1 * ncols, lv->wrap, st, L.nf1 * ncols))) return e;
    }
    // 2. windows in chunks through the stream API's cmvnw + network; raw scores land where the moving average reads them
    float *raw = raw_scores ? raw_scores : scores;
    if (count && n_win) HIP_TRY(hipMemsetAsync(lv->acc, 0, sizeof(int), st));
    for (size_t g0 = 0; g0 < n_win; g0 += win_chunk) {
        const int c = (int)std::min(win_chunk, n_win - g0);
        int rc = kws_launch_live_gather(first_rows, slot_rows, lv->kept, lv->meta, A, (long long)g0, c, L.nf0, L.nf1, L.ring_rows, lv->keep, (int)L.k_full,
                                        rows, ncols, lv->win, st);
        if (rc) return fail(KWS_ERROR_HIP, "live gather kernel launch failed: %s", hipGetErrorString((hipError_t)rc));
        if (fast) e = cmvn_nn_fast_device(h, lv->win, c, raw + g0 * C, st, 0, 0);
        else e = cmvn_nn_device(h, lv->win, c, nullptr, nullptr, raw + g0 * C, nullptr, nullptr, nullptr, st);
        if (e) return e;
        if (count && (rc = kws_launch_scan_count(h->d_flags, h->d_flags2, lv->acc, 0, st)))
            return fail(KWS_ERROR_HIP, "live count kernel launch failed: %s", hipGetErrorString((hipError_t)rc));
    }
    if (count && n_win) {
        int rc = kws_launch_scan_count(h->d_flags, h->d_flags2, lv->acc, 1, st);
        if (rc) return fail(KWS_ERROR_HIP, "live count kernel launch failed: %s", hipGetErrorString((hipError_t)rc));
    }
    // 3. the continuing streams' carry and retained rows (after every read of the old ones above)
    int rc = kws_launch_live_commit(pcm, first_rows, slot_rows, lv->meta, A, sl, lv->cap, L.nf0, L.nf1, lv->keep, ncols, lv->carry, lv->kept, st);
    if (rc) return fail(KWS_ERROR_HIP, "live commit kernel launch failed: %s", hipGetErrorString((hipError_t)rc));
    // 4. the moving average, resumed per (stream, label)
    if (n_win && (rc = kws_launch_live_maf(raw, scores, lv->meta, A, (int)C, (int)L.k_full, lv->maf, st)))
        return fail(KWS_ERROR_HIP, "live moving-average kernel launch failed: %s", hipGetErrorString((hipError_t)rc));
    commit_mirrors();
    return EI_IMPULSE_OK;
}

#pragma GCC visibility pop
}
