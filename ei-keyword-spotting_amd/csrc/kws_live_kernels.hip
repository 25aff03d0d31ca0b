// kws_live_kernels.hip -- the small kernels of kws_live_push_device (kws_live.cpp): live streams in continuous mode, state in HBM between calls.
//   kws_live_stage_kernel    assembles the slices a push finishes, each from the stream's carried samples and the pushed chunk, into aligned
//                            [items][slice] rows for the spectral kernels, plus each slice's pre-emphasis x[-1] from whichever source holds it
//   kws_live_gather_kernel   window w of a stream = its cepstral rows [w nf1, w nf1 + ring_rows) (retained rows of earlier pushes, then the
//                            rows this push computed), then zero rows: [chunk][F]
//   kws_live_commit_kernel   after the gathers: each continuing stream's carried samples and retained rows take the push's new tail
//   kws_live_maf_kernel      run_moving_average_filter (ei_run_classifier.h:134-145) per (stream, label), resumed from the state in HBM
// A stream's samples are numbered from its start (create, reset or finish).  Its carry is a ring of `cap` samples, sample p in slot p % cap,
// holding the samples [k0 slice, n0) not yet part of a finished slice (fewer than cap = slice + grow); its retained rows are a ring of
// `keep` rows, row r in slot r % keep, holding the last min(rows, keep) rows (keep = ring_rows - nf1: what the next window reuses).  Rings
// mean nothing already stored moves: the commit writes only the push's own new samples and rows, into slots no live value occupies.
// Nothing here rounds except the int16 -> float of the wrap sample (kws_mfcc_kernel's product) and the moving average (kws_maf_kernel's
// operations, in its order).
#include "kws_device.h"
#include "kws_window_kernels.h"

#include "../../include/kws/ei_compat.h"

#define KWS_LIVE_TAPS (EI_CLASSIFIER_SLICES_PER_MODEL_WINDOW >> 1)

// (KwsLiveMeta, the per-entry tables of one push, and live_meta: kws_window_kernels.h)

// first = 1: item g is the slice 0 of the entry with fbase[a] <= g < fbase[a + 1]; first = 0: item g is a slice k >= 1, counted over the
// entries in order from each entry's first new slice max(k0, 1).  One block per item.
__global__ void kws_live_stage_kernel(const int16_t *__restrict__ pcm, const int16_t *__restrict__ carry, KwsLiveMeta m, int n_act, long long item0,
                                      int n_items, int first, int slice, int grow, int cap, int16_t *__restrict__ stage, float *__restrict__ wrap)
{
    const long long *prefix = first ? m.fbase : m.ibase;
    for (int j = blockIdx.x; j < n_items; j += gridDim.x) {
        const long long g = item0 + j;
        const int a = kws_prefix_owner(prefix, n_act, g);
        const long long k = first ? 0 : (m.k0[a] > 1 ? m.k0[a] : 1) + (g - prefix[a]);
        const long long n0 = m.n0[a], n1 = n0 + m.len[a];
        const long long base = m.off[a] - n0;                         // pcm[base + p]: stream position p >= n0, in the chunk
        const int16_t *ring = carry + (size_t)m.stream[a] * cap;
        int16_t *dst = stage + (size_t)j * slice;
        const long long p0 = k * slice;
        for (int i = threadIdx.x; i < slice; i += blockDim.x) {
            const long long p = p0 + i;
            dst[i] = p < n0 ? ring[p % cap] : pcm[base + p];
        }
        if (!first && threadIdx.x == 0) {
            // get_data(total_length - 1, 1) of the grown slice: the stream's sample there; past the end of a finished stream a refused read (0)
            const long long p = p0 + slice + grow - 1;
            wrap[j] = p < n1 ? (float)(p < n0 ? ring[p % cap] : pcm[base + p]) * (1.0f / 32768.0f) : 0.0f;
        }
    }
}

// Row r of entry a's stream: retained (r below the rows of its k0 finished slices), else computed by this push (slice 0's rows in first_rows,
// the later slices' rows in slot_rows, nf1 each, from the entry's first new slice on).
__device__ __forceinline__ const float *live_row(const float *__restrict__ first_rows, const float *__restrict__ slot_rows, const float *__restrict__ kept,
                                                 const KwsLiveMeta &m, int a, long long r, int nf0, int nf1, int keep, int ncols)
{
    const long long k0 = m.k0[a];
    const long long t0 = k0 ? nf0 + (k0 - 1) * nf1 : 0;
    if (r < t0) return kept + ((size_t)m.stream[a] * keep + (size_t)(r % keep)) * ncols;
    if (r < nf0) return first_rows + ((size_t)m.fbase[a] * nf0 + (size_t)r) * ncols;
    const long long s0 = (k0 > 1 ? k0 : 1) - 1;                      // slices k >= 1 before the entry's first new one
    return slot_rows + ((size_t)m.ibase[a] * nf1 + (size_t)(r - nf0 - s0 * nf1)) * ncols;
}

// One block per window of the chunk [win0, win0 + n_win) of the push's windows.  The stream's window index is its windows before the push
// (k0 - k_full when positive) plus the window's place among the entry's.
__global__ void kws_live_gather_kernel(const float *__restrict__ first_rows, const float *__restrict__ slot_rows, const float *__restrict__ kept,
                                       KwsLiveMeta m, int n_act, long long win0, int n_win, int nf0, int nf1, int ring_rows, int keep, int k_full,
                                       int rows, int ncols, float *__restrict__ out)
{
    const int per = rows * ncols;
    for (int j = blockIdx.x; j < n_win; j += gridDim.x) {
        const long long g = win0 + j;
        const int a = kws_prefix_owner(m.wbase, n_act, g);
        const long long w = (m.k0[a] > k_full ? m.k0[a] - k_full : 0) + (g - m.wbase[a]);
        float *dst = out + (size_t)j * per;
        for (int e = threadIdx.x; e < per; e += blockDim.x) {
            const int i = e / ncols, c = e - i * ncols;
            dst[e] = i < ring_rows ? live_row(first_rows, slot_rows, kept, m, a, w * nf1 + i, nf0, nf1, keep, ncols)[c] : 0.0f;   // rows the reference never writes: 0
        }
    }
}

// One block per entry.  A stream the push does not finish keeps the samples [k1 slice, n1) and its last min(rows, keep) rows: the ring slots
// of the push's new samples [max(n0, k1 slice), n1) and new rows [max(t0, t1 - keep), t1) are written; every other slot keeps its value.
// Runs after every stage and gather launch of the push (they read the slots this overwrites).
__global__ void kws_live_commit_kernel(const int16_t *__restrict__ pcm, const float *__restrict__ first_rows, const float *__restrict__ slot_rows,
                                       KwsLiveMeta m, int n_act, int slice, int cap, int nf0, int nf1, int keep, int ncols, int16_t *__restrict__ carry,
                                       float *__restrict__ kept)
{
    for (int a = blockIdx.x; a < n_act; a += gridDim.x) {
        if (m.fin[a]) continue;
        const long long n0 = m.n0[a], n1 = n0 + m.len[a], k0 = m.k0[a], k1 = m.k1[a];
        const long long base = m.off[a] - n0;
        int16_t *ring = carry + (size_t)m.stream[a] * cap;
        const long long c0 = k1 * slice > n0 ? k1 * slice : n0;
        for (long long p = c0 + threadIdx.x; p < n1; p += blockDim.x) ring[p % cap] = pcm[base + p];
        if (keep <= 0 || k1 == k0) continue;
        const long long t0 = k0 ? nf0 + (k0 - 1) * nf1 : 0, t1 = nf0 + (k1 - 1) * nf1;
        const long long r0 = t1 - keep > t0 ? t1 - keep : t0;
        float *dst = kept + (size_t)m.stream[a] * keep * ncols;
        for (long long e = threadIdx.x; e < (t1 - r0) * ncols; e += blockDim.x) {
            const long long r = r0 + e / ncols;
            const int c = (int)(e - (r - r0) * ncols);
            dst[(size_t)(r % keep) * ncols + c] = live_row(first_rows, slot_rows, kept, m, a, r, nf0, nf1, keep, ncols)[c];
        }
    }
}

// raw [windows][labels] -> scores (may be the same buffer), one thread per (entry, label).  The filter state of stream s, label l is
// maf[(s labels + l) (taps + 1) + i]: taps buf[i], then the running sum; its index is the stream's window count mod taps.  A stream with no
// window before the push starts from the fresh filter (which is how finish and reset zero it); a finished stream's filter is not stored.
__global__ void kws_live_maf_kernel(const float *raw, float *scores, KwsLiveMeta m, int n_act, int labels, int k_full, float *__restrict__ maf)
{
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_act * labels) return;
    const int a = t / labels, l = t - a * labels;
    const long long g0 = m.wbase[a], g1 = m.wbase[a + 1];
    if (g0 == g1) return;
    const long long w0 = m.k0[a] > k_full ? m.k0[a] - k_full : 0;
    float *st = maf + ((size_t)m.stream[a] * labels + l) * (KWS_LIVE_TAPS + 1);
    float buf[KWS_LIVE_TAPS];
    float rs = 0.0f;
#pragma unroll
    for (int i = 0; i < KWS_LIVE_TAPS; ++i) buf[i] = w0 ? st[i] : 0.0f;
    if (w0) rs = st[KWS_LIVE_TAPS];
    int idx = (int)(w0 % KWS_LIVE_TAPS);
    for (long long g = g0; g < g1; ++g) {
        const float v = raw[(size_t)g * labels + l];
        rs -= buf[idx];
        rs += v;
        buf[idx] = v;
        scores[(size_t)g * labels + l] = rs / (float)KWS_LIVE_TAPS;
        if (++idx >= KWS_LIVE_TAPS) idx = 0;
    }
    if (m.fin[a]) return;
#pragma unroll
    for (int i = 0; i < KWS_LIVE_TAPS; ++i) st[i] = buf[i];
    st[KWS_LIVE_TAPS] = rs;
}

int kws_launch_live_stage(const int16_t *pcm, const int16_t *carry, const long long *meta, int n_act, long long item0, int n_items, int first, int slice,
                          int grow, int cap, int16_t *stage, float *wrap, hipStream_t stream)
{
    (void)hipGetLastError();
    if (n_items <= 0) return 0;
    hipLaunchKernelGGL(kws_live_stage_kernel, dim3(n_items < 65536 ? n_items : 65536), dim3(256), 0, stream, pcm, carry, live_meta(meta, n_act), n_act,
                       item0, n_items, first, slice, grow, cap, stage, wrap);
    return (int)hipGetLastError();
}

int kws_launch_live_gather(const float *first_rows, const float *slot_rows, const float *kept, const long long *meta, int n_act, long long win0, int n_win,
                           int nf0, int nf1, int ring_rows, int keep, int k_full, int rows, int ncols, float *out, hipStream_t stream)
{
    (void)hipGetLastError();
    if (n_win <= 0) return 0;
    hipLaunchKernelGGL(kws_live_gather_kernel, dim3(n_win < 65536 ? n_win : 65536), dim3(256), 0, stream, first_rows, slot_rows, kept, live_meta(meta, n_act),
                       n_act, win0, n_win, nf0, nf1, ring_rows, keep, k_full, rows, ncols, out);
    return (int)hipGetLastError();
}

int kws_launch_live_commit(const int16_t *pcm, const float *first_rows, const float *slot_rows, const long long *meta, int n_act, int slice, int cap, int nf0,
                           int nf1, int keep, int ncols, int16_t *carry, float *kept, hipStream_t stream)
{
    (void)hipGetLastError();
    if (n_act <= 0) return 0;
    hipLaunchKernelGGL(kws_live_commit_kernel, dim3(n_act < 65536 ? n_act : 65536), dim3(256), 0, stream, pcm, first_rows, slot_rows, live_meta(meta, n_act),
                       n_act, slice, cap, nf0, nf1, keep, ncols, carry, kept);
    return (int)hipGetLastError();
}

int kws_launch_live_maf(const float *raw, float *scores, const long long *meta, int n_act, int labels, int k_full, float *maf, hipStream_t stream)
{
    (void)hipGetLastError();
    const int n = n_act * labels;
    if (n <= 0) return 0;
    hipLaunchKernelGGL(kws_live_maf_kernel, dim3((n + 63) / 64), dim3(64), 0, stream, raw, scores, live_meta(meta, n_act), n_act, labels, k_full, maf);
    return (int)hipGetLastError();
}
