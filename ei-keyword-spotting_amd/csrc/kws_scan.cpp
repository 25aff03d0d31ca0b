// kws_scan.cpp -- whole recordings in continuous mode (kws_scan_window_count, kws_scan_recordings_device; contract in include/kws/kws.h).
//
// A fresh kws_stream_batch fed one recording slice by slice writes slice 0's nf0 cepstral rows, then nf1 rows per slice, into one
// rolling buffer; from the step where the buffer is full (ring_rows rows written) every step produces a window.  Read as one contiguous
// row array per recording, window w is rows [w nf1, w nf1 + ring_rows) followed by the rows the reference never writes (zeros).  The
// rows of a slice depend only on its own samples and its wrap sample, so every slice of the call is independent work:
//   1. front end: slices copied from the recordings into aligned rows (kws_scan_stage_kernel), then the spectral kernels the stream API
//      runs (spectral_device) -- slice 0 of every recording into first_rows [A][nf0][cols], the slices k >= 1 into slot_rows, nf1 rows
//      each, recording after recording: together the contiguous row arrays;
//   2. windows gathered in chunks into [chunk][F] (kws_scan_gather_kernel) for the stream API's cmvnw + network (cmvn_nn_device, or
//      cmvn_nn_fast_device in KWS_MODE_FAST), which write each window's raw scores in place;
//   3. the moving average per (recording, label) over its windows in order (kws_scan_maf_kernel).
// A = the recordings of the call that produce at least one window; the others need no work.
// Steps 2 and 3 end in callables (kws_scan_run: the finishing hook per chunk, the moving-average hook): what is written above is what
// kws_scan_recordings_device passes; a bank passes cmvnw once + every member's network and one filter launch for all (kws_bank_windows.cpp).
// Scratch and its bounds, the table upload, the finishing step of a chunk and the fast counters: the window pipelines' core, kws_windows.h.
#include "kws_internal.h"
#include "kws_windows.h"

int kws_launch_scan_stage(const int16_t *pcm, const long long *off, const long long *len, const long long *ibase, int n_rec, long long item0, int n_items,
                          int first, int slice, int grow, int16_t *stage, float *wrap, hipStream_t stream);
int kws_launch_scan_gather(const float *first_rows, const float *slot_rows, const long long *wbase, const long long *ibase, int n_rec, long long win0,
                           int n_win, int nf0, int nf1, int ring_rows, int rows, int ncols, float *out, hipStream_t stream);
int kws_launch_scan_maf(const float *raw, float *scores, const long long *wbase, int n_rec, int labels, hipStream_t stream);

static void scan_release(kws_handle *h)
{
    if (!h->scan) return;
    h->scan->release();
    delete h->scan;
    h->scan = nullptr;
}

// (ScanLayout: kws_internal.h; the live sessions of kws_live.cpp share it)
EI_IMPULSE_ERROR scan_layout(const kws_handle *h, size_t slice_samples, ScanLayout *L)
{
    const Model &m = h->model;
    const size_t F = m.nn_input_frame_size;
    const int frame_len = h->dsp.frame_len, stride = h->dsp.frame_stride, ncols = h->dsp.n_cepstral;
    const size_t grown_by = (size_t)(m.dsp.frame_length * (float)m.frequency);
    size_t slice_offset = 0;
    bool full = false;
    int ring_rows = 0;
    L->grow = (int)grown_by;
    for (size_t k = 0;; ++k) {
        const size_t n_claimed = slice_samples + (k > 0 ? grown_by : 0);
        const int nf = n_claimed >= (size_t)frame_len ? (int)floorf((float)(n_claimed - (size_t)frame_len) / (float)stride) : 0;
        const size_t feature_size = (size_t)(nf > 0 ? nf : 0) * (size_t)ncols;
        if (nf < 1 || (!h->dsp.generic && nf > kws_mfcc_max_frames(h->dsp.n_filters)) || feature_size > F || slice_offset + feature_size > F ||
            (size_t)(nf - 1) * stride + std::min(h->dsp.fft_len, frame_len) > slice_samples || (!h->dsp.generic && (slice_samples * 2) % 16 != 0))
            return fail(EI_IMPULSE_DSP_ERROR, "slice of %zu samples (claimed %zu) yields %d frames", slice_samples, n_claimed, nf);
        const int row0 = (int)(slice_offset / (size_t)ncols);
        if (ring_rows && row0 + nf != ring_rows)
            return fail(EI_IMPULSE_DSP_ERROR, "slice of %d frames in a window laid out for slices of %d", nf, ring_rows - row0);
        if (k == 0) L->nf0 = nf; else L->nf1 = nf;
        if (full) break;                                   // a steady step has been checked: every later step is the same
        slice_offset += feature_size;
        if (slice_offset > F - feature_size) {
            full = true;
            slice_offset -= feature_size;
            ring_rows = (int)((slice_offset + feature_size) / (size_t)ncols);
            L->k_full = k;
        }
    }
    L->ring_rows = ring_rows;
    return EI_IMPULSE_OK;
}

// The finishing and moving-average steps of kws_scan_recordings_device itself: cmvnw + the handle's network in the handle's mode, chunk by
// chunk, raw scores where the moving average reads them; then one fresh filter per recording (h->mu held)
struct ScanOwn {
    float *scores, *raw;
    KwsChunkCounts counts;
    bool started = false;
};
static EI_IMPULSE_ERROR scan_own_finish(void *ctx, float *win, size_t n, size_t g0, hipStream_t st)
{
    ScanOwn &o = *(ScanOwn *)ctx;
    kws_handle *h = o.counts.h;
    EI_IMPULSE_ERROR e;
    if (!o.started) {
        o.started = true;
        o.counts = KwsChunkCounts(h);                              // (the handle's mode, read under its lock)
        if ((e = o.counts.begin(h->scan->acc, n, st))) return e;
    }
    if (n == 0) return o.counts.end(st);                           // after the last chunk
    if ((e = kws_finish_window_chunk(h, win, n, o.raw + g0 * h->model.labels.size(), nullptr, o.counts.fast, st))) return e;
    return o.counts.chunk(st);
}
static EI_IMPULSE_ERROR scan_own_maf(void *ctx, const long long *wbase, int n_rec, hipStream_t st)
{
    ScanOwn &o = *(ScanOwn *)ctx;
    KWS_LAUNCH_TRY("scan moving-average kernel", kws_launch_scan_maf(o.raw, o.scores, wbase, n_rec, (int)o.counts.h->model.labels.size(), st));
    return EI_IMPULSE_OK;
}

// The scan: argument checks, staging and cepstral rows, windows gathered in chunks; every chunk (win [n][F] cepstra before cmvnw, the call's
// windows g0 .. g0 + n - 1) goes to finish(), which is called once more with n == 0 after the last chunk; then maf() (kws_internal.h).
EI_IMPULSE_ERROR kws_scan_run(kws_handle *h, const int16_t *pcm, const size_t *offsets, const size_t *lengths, size_t R, size_t slice_samples, size_t labels,
                              int take_lock, kws_slide_finish_fn finish, kws_window_maf_fn maf, void *ctx, hipStream_t st)
{
    if (R > 0 && (!pcm || !offsets || !lengths)) return fail(KWS_ERROR_BAD_ARGUMENT, "null argument");
    if (R > 0x3fffffff) return fail(KWS_ERROR_BAD_ARGUMENT, "too many recordings");
    ScanLayout L;
    EI_IMPULSE_ERROR e = scan_layout(h, slice_samples, &L);
    if (e) return e;
    // the recordings that produce windows, and where their windows / slices go
    std::vector<long long> off, len, wbase(1, 0), ibase(1, 0);
    for (size_t r = 0; r < R; ++r) {
        const size_t K = lengths[r] / slice_samples, W = L.windows(K);
        if (!W) continue;
        off.push_back((long long)offsets[r]);
        len.push_back((long long)lengths[r]);
        wbase.push_back(wbase.back() + (long long)W);
        ibase.push_back(ibase.back() + (long long)(K - 1));
    }
    const int A = (int)off.size();
    if (A == 0) return EI_IMPULSE_OK;
    const size_t n_win = (size_t)wbase.back(), n_slots = (size_t)ibase.back();
    const Model &m = h->model;
    const size_t F = m.nn_input_frame_size, C = labels;
    const int ncols = h->dsp.n_cepstral, rows = (int)(F / (size_t)ncols);
    if (n_win * C > (size_t)1 << 40) return fail(KWS_ERROR_BAD_ARGUMENT, "too many windows");
    HIP_TRY(hipSetDevice(h->device));
    std::unique_lock<std::mutex> lk(h->mu, std::defer_lock);
    if (take_lock) lk.lock();
    if (!h->scan) { h->scan = new KwsWindowScratch(); h->scan_release = scan_release; }
    KwsWindowScratch &S = *h->scan;
    const size_t item_cap = kws_window_item_cap(slice_samples), win_chunk = kws_window_chunk(F, n_win);
    const size_t first_floats = (size_t)A * L.nf0 * ncols, rows_floats = first_floats + n_slots * L.nf1 * ncols;
    if ((e = S.reserve(h, item_cap * slice_samples, item_cap, win_chunk * F, rows_floats, 4 * (size_t)A + 2, win_chunk))) return e;
    ScratchUse use(h, st);
    // per-recording tables: off [A], len [A], wbase [A + 1], ibase [A + 1]
    if ((e = kws_upload_tables(S, { &off, &len, &wbase, &ibase }, st))) return e;
    const long long *d_off = S.meta, *d_len = S.meta + A, *d_wbase = S.meta + 2 * A, *d_ibase = S.meta + 3 * A + 1;
    const int slice = (int)slice_samples;
    float *first_rows = S.rows, *slot_rows = S.rows + first_floats;
    // 1. front end: the stream API's spectral launches, on aligned copies of the slices
    KwsDspPlan P0 = h->dsp, P1 = h->dsp;
    P0.n_samples = P1.n_samples = slice;
    P0.n_frames = L.nf0;
    P1.n_frames = L.nf1;
    for (size_t a0 = 0; a0 < (size_t)A; a0 += item_cap) {
        const int n = (int)std::min(item_cap, (size_t)A - a0);
        KWS_LAUNCH_TRY("scan staging kernel", kws_launch_scan_stage(pcm, d_off, d_len, d_ibase, A, (long long)a0, n, 1, slice, L.grow, S.stage, S.wrap, st));
        if ((e = spectral_device(h, P0, S.stage, 0, n, first_rows + a0 * L.nf0 * ncols, nullptr, st, L.nf0 * ncols))) return e;
    }
    for (size_t g0 = 0; g0 < n_slots; g0 += item_cap) {
        const int n = (int)std::min(item_cap, n_slots - g0);
        KWS_LAUNCH_TRY("scan staging kernel", kws_launch_scan_stage(pcm, d_off, d_len, d_ibase, A, (long long)g0, n, 0, slice, L.grow, S.stage, S.wrap, st));
        if ((e = spectral_device(h, P1, S.stage, 0, n, slot_rows + g0 * L.nf1 * ncols, S.wrap, st, L.nf1 * ncols))) return e;
    }
    // 2. windows in chunks through the finishing step (the stream API's cmvnw + network); raw scores land where the moving average reads them
    for (size_t g0 = 0; g0 < n_win; g0 += win_chunk) {
        const int n = (int)std::min(win_chunk, n_win - g0);
        KWS_LAUNCH_TRY("scan gather kernel", kws_launch_scan_gather(first_rows, slot_rows, d_wbase, d_ibase, A, (long long)g0, n, L.nf0, L.nf1, L.ring_rows, rows, ncols, S.win, st));
        if ((e = finish(ctx, S.win, (size_t)n, g0, st))) return e;
    }
    if ((e = finish(ctx, S.win, 0, n_win, st))) return e;
    // 3. the moving average, one fresh filter per recording
    return maf(ctx, d_wbase, A, st);
}

extern "C" {
#pragma GCC visibility push(default)

EI_IMPULSE_ERROR kws_scan_window_count(const kws_handle *h, size_t n_samples, size_t slice_samples, size_t *n_windows)
{
    if (!h || !n_windows) return fail(KWS_ERROR_BAD_ARGUMENT, "null argument");
    *n_windows = 0;
    ScanLayout L;
    EI_IMPULSE_ERROR e = scan_layout(h, slice_samples, &L);
    if (e) return e;
    *n_windows = L.windows(n_samples / slice_samples);
    return EI_IMPULSE_OK;
}

EI_IMPULSE_ERROR kws_scan_recordings_device(kws_handle *h, const int16_t *pcm, const size_t *offsets, const size_t *lengths, size_t R,
                                            size_t slice_samples, float *scores, float *raw_scores, void *stream)
{
    if (!h || !scores) return fail(KWS_ERROR_BAD_ARGUMENT, "null argument");
    ScanOwn own{ scores, raw_scores ? raw_scores : scores, KwsChunkCounts(h) };
    return kws_scan_run(h, pcm, offsets, lengths, R, slice_samples, h->model.labels.size(), 1, scan_own_finish, scan_own_maf, &own, (hipStream_t)stream);
}

#pragma GCC visibility pop
}
