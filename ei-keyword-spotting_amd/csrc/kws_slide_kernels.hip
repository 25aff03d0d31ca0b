// kws_slide_kernels.hip -- the small kernels of kws_slide_recordings_device (kws_slide.cpp): every one-shot window of whole recordings.
//   kws_slide_stage_kernel        copies a chunk of items (pieces of a recording's runs of frames, or whole windows) from any sample offset
//                                 into aligned [items][item_len] rows for the spectral kernels, zeros past the recording's end, plus each
//                                 item's pre-emphasis x[-1]: the sample before the item
//   kws_slide_stage_first_kernel  frame 0 of a chunk of windows, nfi windows per item: window k's first frame at samples [k S1, k S1 + used)
//                                 of the item and, one sample before it, the window's LAST sample -- the predecessor the reference's
//                                 pre-emphasis wraps to (processing.hpp:104-106) -- so that one multi-frame launch yields nfi windows' rows
//   kws_slide_gather_kernel       window w = its frame-0 row + its rows f >= 1, which are contiguous in the recording's row array: [chunk][F]
// The arithmetic of the front end and of the network is the existing kernels'; nothing here rounds except the int16 -> float of the wrap
// sample (the same product as kws_mfcc_kernel's).
#include "kws_device.h"
#include "kws_window_kernels.h"

// n samples from pcm + p (samples at or past `end` read as 0) to dst, dword-wide where both sides allow it.  All threads of the block.
__device__ __forceinline__ void slide_copy(const int16_t *__restrict__ pcm, long long p, long long end, int16_t *__restrict__ dst, int n)
{
    const int16_t *src = pcm + p;
    const int tid = threadIdx.x, nt = blockDim.x;
    if ((((uintptr_t)dst) & 3) != 0) {                             // (windows of an odd length, staged back to back)
        for (int i = tid; i < n; i += nt) dst[i] = p + i < end ? src[i] : (int16_t)0;
        return;
    }
    const int n2 = n >> 1;
    uint32_t *d2 = (uint32_t *)dst;
    if ((((uintptr_t)src) & 3) == 0) {
        const uint32_t *s2 = (const uint32_t *)src;
        for (int i = tid; i < n2; i += nt) {
            const long long q = p + 2 * i;
            uint32_t v = 0;
            if (q + 1 < end) v = s2[i];
            else if (q < end) v = (uint16_t)src[2 * i];
            d2[i] = v;
        }
    } else {
        for (int i = tid; i < n2; i += nt) {
            const long long q = p + 2 * i;
            const uint32_t lo = q < end ? (uint16_t)src[2 * i] : 0u, hi = q + 1 < end ? (uint16_t)src[2 * i + 1] : 0u;
            d2[i] = lo | (hi << 16);
        }
    }
    if ((n & 1) && tid == 0) dst[n - 1] = p + n - 1 < end ? src[n - 1] : (int16_t)0;
}

// Item item0 + j belongs to slot s = the last one with ibase[s] <= item (ibase: items of the slots before, n_slots + 1 entries); it is the
// slot's k-th item and starts at sample src[s] + (k / ips) seg_pitch + (k % ips) item_adv of pcm (ips: items per segment of the slot; a slot
// that is one run has one segment).  end[s]: the sample after the slot's recording.  has_wrap = 0: wrap = 0, nothing before the item is read.
// One block per item.
__global__ void kws_slide_stage_kernel(const int16_t *__restrict__ pcm, const long long *__restrict__ src, const long long *__restrict__ end,
                                       const long long *__restrict__ ibase, int n_slots, long long item0, int n_items, long long ips,
                                       long long seg_pitch, long long item_adv, int item_len, int has_wrap, int16_t *__restrict__ stage,
                                       float *__restrict__ wrap)
{
    for (int j = blockIdx.x; j < n_items; j += gridDim.x) {
        const long long g = item0 + j;
        const int s = kws_prefix_owner(ibase, n_slots, g);
        const long long k = g - ibase[s], seg = k / ips;
        const long long p = src[s] + seg * seg_pitch + (k - seg * ips) * item_adv;
        slide_copy(pcm, p, end[s], stage + (size_t)j * item_len, item_len);
        if (wrap && threadIdx.x == 0) wrap[j] = has_wrap ? (float)pcm[p - 1] * (1.0f / 32768.0f) : 0.0f;
    }
}

// Item m holds frame 0 of the windows win0 + m nfi + k, k < nfi (windows past win0 + n_win: zeros).  off[a]: recording a's first sample in
// pcm; wbase: windows of the recordings before (n_rec + 1 entries).  Slot k of an item is S1 samples: the frame's `used` samples, zeros, and
// in its last sample the predecessor of slot k + 1's frame; slot 0's predecessor goes to wrap[m].  One block per item.
__global__ void kws_slide_stage_first_kernel(const int16_t *__restrict__ pcm, const long long *__restrict__ off, const long long *__restrict__ wbase,
                                             int n_rec, long long win0, int n_win, int n_items, int nfi, int S1, int used, long long hop, int clip,
                                             int16_t *__restrict__ stage, float *__restrict__ wrap)
{
    for (int m = blockIdx.x; m < n_items; m += gridDim.x) {
        int16_t *item = stage + (size_t)m * nfi * S1;
        // the window of slot k: where it starts in pcm (-1: no such window)
        auto start_of = [&](int k) -> long long {
            const long long j = (long long)m * nfi + k;
            if (k >= nfi || j >= n_win) return -1;
            const int a = kws_prefix_owner(wbase, n_rec, win0 + j);
            return off[a] + (win0 + j - wbase[a]) * hop;
        };
        long long p = start_of(0);
        if (threadIdx.x == 0) wrap[m] = p >= 0 ? (float)pcm[p + clip - 1] * (1.0f / 32768.0f) : 0.0f;
        for (int k = 0; k < nfi; k++) {
            const long long pn = start_of(k + 1);
            int16_t *dst = item + (size_t)k * S1;
            // a frame lies inside its window: no read past p + clip
            slide_copy(pcm, p >= 0 ? p : 0, p >= 0 ? p + used : 0, dst, S1 - 1);
            if (threadIdx.x == 0) dst[S1 - 1] = pn >= 0 ? pcm[pn + clip - 1] : (int16_t)0;
            p = pn;
        }
    }
}

// One block per window of the chunk.  Window w of recording a sits in the recording's slot t = w % phases as its (w / phases)-th window:
// its rows f >= pre are rows [ibase[sbase[a] + t] nfi + (w / phases) pitch, + nf - pre) of `rows`; its row 0 (pre = 1) is row j of `first`.
__global__ void kws_slide_gather_kernel(const float *__restrict__ rows, const float *__restrict__ first, const long long *__restrict__ wbase,
                                        const long long *__restrict__ sbase, const long long *__restrict__ ibase, int n_rec, long long win0, int n_win,
                                        long long phases, long long pitch, int nfi, int pre, int nf, int ncols, float *__restrict__ out)
{
    const int n_first = pre * ncols, n_rest = (nf - pre) * ncols;
    for (int j = blockIdx.x; j < n_win; j += gridDim.x) {
        float *dst = out + (size_t)j * (n_first + n_rest);
        if (n_rest > 0) {
            const long long g = win0 + j;
            const int a = kws_prefix_owner(wbase, n_rec, g);
            const long long w = g - wbase[a], i = phases > 1 ? w / phases : w, t = w - i * phases;
            const float *src = rows + (size_t)(ibase[sbase[a] + t] * nfi + i * pitch) * ncols;
            for (int e = threadIdx.x; e < n_rest; e += blockDim.x) dst[n_first + e] = src[e];
        }
        if (threadIdx.x < n_first) dst[threadIdx.x] = first[(size_t)j * ncols + threadIdx.x];
    }
}

int kws_launch_slide_stage(const int16_t *pcm, const long long *src, const long long *end, const long long *ibase, int n_slots, long long item0,
                           int n_items, long long ips, long long seg_pitch, long long item_adv, int item_len, int has_wrap, int16_t *stage, float *wrap,
                           hipStream_t stream)
{
    (void)hipGetLastError();
    if (n_items <= 0) return 0;
    hipLaunchKernelGGL(kws_slide_stage_kernel, dim3(n_items < 65536 ? n_items : 65536), dim3(256), 0, stream, pcm, src, end, ibase, n_slots, item0,
                       n_items, ips, seg_pitch, item_adv, item_len, has_wrap, stage, wrap);
    return (int)hipGetLastError();
}

int kws_launch_slide_stage_first(const int16_t *pcm, const long long *off, const long long *wbase, int n_rec, long long win0, int n_win, int nfi, int S1,
                                 int used, long long hop, int clip, int16_t *stage, float *wrap, hipStream_t stream)
{
    (void)hipGetLastError();
    if (n_win <= 0) return 0;
    const int n_items = (n_win + nfi - 1) / nfi;
    hipLaunchKernelGGL(kws_slide_stage_first_kernel, dim3(n_items < 65536 ? n_items : 65536), dim3(256), 0, stream, pcm, off, wbase, n_rec, win0, n_win,
                       n_items, nfi, S1, used, hop, clip, stage, wrap);
    return (int)hipGetLastError();
}

int kws_launch_slide_gather(const float *rows, const float *first, const long long *wbase, const long long *sbase, const long long *ibase, int n_rec,
                            long long win0, int n_win, long long phases, long long pitch, int nfi, int pre, int nf, int ncols, float *out,
                            hipStream_t stream)
{
    (void)hipGetLastError();
    if (n_win <= 0) return 0;
    hipLaunchKernelGGL(kws_slide_gather_kernel, dim3(n_win < 65536 ? n_win : 65536), dim3(256), 0, stream, rows, first, wbase, sbase, ibase, n_rec, win0,
                       n_win, phases, pitch, nfi, pre, nf, ncols, out);
    return (int)hipGetLastError();
}
