// kws_scan_kernels.hip -- the small kernels of kws_scan_recordings_device (kws_scan.cpp): whole recordings in continuous mode.
//   kws_scan_stage_kernel    copies the slices of a chunk of (recording, slice) items from any sample offset into aligned [items][slice]
//                            rows for the spectral kernels, plus each slice's pre-emphasis x[-1] read from the recording (or 0 past its end)
//   kws_scan_gather_kernel   window w of a recording = its contiguous cepstral rows [w nf1, w nf1 + ring_rows), then zero rows: [chunk][F]
//   kws_scan_maf_kernel      run_moving_average_filter (ei_run_classifier.h:134-145) per (recording, label), window after window
// The arithmetic of the front end and of the network is the existing kernels'; nothing here rounds except the int16 -> float of the wrap
// sample (the same product as kws_mfcc_kernel's) and the moving average (kws_maf_kernel's operations, in its order).
#include "kws_device.h"
#include "kws_window_kernels.h"

#include "../../include/kws/ei_compat.h"

#define KWS_SCAN_TAPS (EI_CLASSIFIER_SLICES_PER_MODEL_WINDOW >> 1)

// first = 1: item j of the chunk is slice 0 of recording item0 + j; first = 0: item j is the (item0 + j)-th slice k >= 1 of the call, counted
// over the recordings in order (ibase[a] = slices k >= 1 of the recordings before a).  One block per item.
__global__ void kws_scan_stage_kernel(const int16_t *__restrict__ pcm, const long long *__restrict__ off, const long long *__restrict__ len,
                                      const long long *__restrict__ ibase, int n_rec, long long item0, int n_items, int first, int slice, int grow,
                                      int16_t *__restrict__ stage, float *__restrict__ wrap)
{
    for (int j = blockIdx.x; j < n_items; j += gridDim.x) {
        int a;
        long long k;
        if (first) { a = (int)(item0 + j); k = 0; }
        else {
            const long long g = item0 + j;
            a = kws_prefix_owner(ibase, n_rec, g);
            k = 1 + g - ibase[a];
        }
        const int16_t *src = pcm + off[a] + k * (long long)slice;
        int16_t *dst = stage + (size_t)j * slice;
        for (int i = threadIdx.x; i < slice; i += blockDim.x) dst[i] = src[i];
        if (!first && threadIdx.x == 0) {
            // get_data(total_length - 1, 1) of the grown slice: inside the recording its sample, past its end a refused read (0)
            const long long p = k * slice + slice + grow - 1;
            wrap[j] = p < len[a] ? (float)pcm[off[a] + p] * (1.0f / 32768.0f) : 0.0f;
        }
    }
}

// One block per window.  wbase / ibase: windows / slices k >= 1 of the recordings before a (n_rec + 1 entries).
__global__ void kws_scan_gather_kernel(const float *__restrict__ first_rows, const float *__restrict__ slot_rows, const long long *__restrict__ wbase,
                                       const long long *__restrict__ ibase, int n_rec, long long win0, int n_win, int nf0, int nf1, int ring_rows, int rows,
                                       int ncols, float *__restrict__ out)
{
    const int per = rows * ncols;
    for (int j = blockIdx.x; j < n_win; j += gridDim.x) {
        const long long g = win0 + j;
        const int a = kws_prefix_owner(wbase, n_rec, g);
        const long long w = g - wbase[a];
        float *dst = out + (size_t)j * per;
        for (int e = threadIdx.x; e < per; e += blockDim.x) {
            const int i = e / ncols, c = e - i * ncols;
            float v = 0.0f;                                       // rows the reference never writes
            if (i < ring_rows) {
                const long long r = w * nf1 + i;                  // row of the recording's contiguous row array
                v = r < nf0 ? first_rows[((size_t)a * nf0 + r) * ncols + c] : slot_rows[((size_t)ibase[a] * nf1 + (r - nf0)) * ncols + c];
            }
            dst[e] = v;
        }
    }
}

// raw [windows][labels] -> scores (may be the same buffer): a fresh filter per recording, kws_maf_kernel's operations in its order
__global__ void kws_scan_maf_kernel(const float *raw, float *scores, const long long *__restrict__ wbase, int n_rec, int labels)
{
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_rec * labels) return;
    const int a = t / labels, l = t - a * labels;
    float buf[KWS_SCAN_TAPS];
#pragma unroll
    for (int i = 0; i < KWS_SCAN_TAPS; ++i) buf[i] = 0.0f;
    float rs = 0.0f;
    int idx = 0;
    for (long long g = wbase[a]; g < wbase[a + 1]; ++g) {
        const float v = raw[(size_t)g * labels + l];
        rs -= buf[idx];
        rs += v;
        buf[idx] = v;
        scores[(size_t)g * labels + l] = rs / (float)KWS_SCAN_TAPS;
        if (++idx >= KWS_SCAN_TAPS) idx = 0;
    }
}

// fast mode: the windows each chunk's guard handed back, summed over the chunks of a call; finish = 1 publishes the sum as the call's counts
__global__ void kws_scan_count_kernel(int *flags, int *flags2, int *acc, int finish)
{
    if (finish) { flags[0] = acc[0]; flags2[0] = acc[0]; }
    else acc[0] += flags[0];
}

int kws_launch_scan_stage(const int16_t *pcm, const long long *off, const long long *len, const long long *ibase, int n_rec, long long item0, int n_items,
                          int first, int slice, int grow, int16_t *stage, float *wrap, hipStream_t stream)
{
    (void)hipGetLastError();
    if (n_items <= 0) return 0;
    hipLaunchKernelGGL(kws_scan_stage_kernel, dim3(n_items < 65536 ? n_items : 65536), dim3(256), 0, stream, pcm, off, len, ibase, n_rec, item0, n_items,
                       first, slice, grow, stage, wrap);
    return (int)hipGetLastError();
}

int kws_launch_scan_gather(const float *first_rows, const float *slot_rows, const long long *wbase, const long long *ibase, int n_rec, long long win0,
                           int n_win, int nf0, int nf1, int ring_rows, int rows, int ncols, float *out, hipStream_t stream)
{
    (void)hipGetLastError();
    if (n_win <= 0) return 0;
    hipLaunchKernelGGL(kws_scan_gather_kernel, dim3(n_win < 65536 ? n_win : 65536), dim3(256), 0, stream, first_rows, slot_rows, wbase, ibase, n_rec,
                       win0, n_win, nf0, nf1, ring_rows, rows, ncols, out);
    return (int)hipGetLastError();
}

int kws_launch_scan_maf(const float *raw, float *scores, const long long *wbase, int n_rec, int labels, hipStream_t stream)
{
    (void)hipGetLastError();
    const int n = n_rec * labels;
    if (n <= 0) return 0;
    hipLaunchKernelGGL(kws_scan_maf_kernel, dim3((n + 63) / 64), dim3(64), 0, stream, raw, scores, wbase, n_rec, labels);
    return (int)hipGetLastError();
}

int kws_launch_scan_count(int *flags, int *flags2, int *acc, int finish, hipStream_t stream)
{
    (void)hipGetLastError();
    hipLaunchKernelGGL(kws_scan_count_kernel, dim3(1), dim3(1), 0, stream, flags, flags2, acc, finish);
    return (int)hipGetLastError();
}
