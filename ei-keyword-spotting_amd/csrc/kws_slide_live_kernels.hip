// kws_slide_live_kernels.hip -- the small kernels of kws_slide_live_push_device (kws_slide_live.cpp): live streams of one-shot windows,
// state in HBM between calls.
//   kws_slide_live_stage_rows_kernel  the cepstral rows a push needs and no earlier push has computed, each an independent (stream, sample
//                                     position) frame with its own pre-emphasis predecessor -- a new shared position (predecessor: the sample
//                                     before it) or frame 0 of a completed window (predecessor: the window's LAST sample, processing.hpp:104-106)
//                                     -- packed nfi to an item in kws_slide_stage_first_kernel's layout: frame k at samples [k S1, k S1 + used)
//                                     of the item, zeros, and in the slot's last sample the predecessor of frame k + 1; frame 0's goes to wrap[]
//   kws_slide_live_stage_clips_kernel the direct path: every completed window as an aligned clip
//   kws_slide_live_gather_kernel      window w = its frame-0 row + its rows f >= pre, each from the stream's retained ring (positions computed
//                                     by earlier pushes) or from this push's new rows: [chunk][F]
//   kws_slide_live_commit_kernel      after every read of the old state: each entry's new carried samples and last retained rows
// A stream's samples are numbered from its start (create or reset).  Its carry is a ring of `cap` = clip samples, sample p in slot p % cap,
// holding the samples from the next incomplete window's start up to the stream's end; its retained rows are a ring of `run` = frames - pre
// rows, shared position j (the frame at sample (j + pre) stride) in slot j % run.  A sample of the stream is read from the ring below n0 (the
// stream's length before the push) and from the pushed chunk from n0 on.  Ring slots are stepped, not divided: one 64-bit remainder per block.
// The arithmetic of the front end and of the network is the existing kernels'; nothing here rounds except the int16 -> float of the wrap
// sample (the same product as kws_slide_stage_kernel's).
#include "kws_device.h"
#include "kws_window_kernels.h"

// The per-entry tables of one push, n_act entries (the entries of the call with device work), each a device array:
struct KwsSlideLiveMeta {
    const long long *off;      // the entry's chunk: pcm + off
    const long long *n0;       // samples the stream had before the push
    const long long *len;      // samples pushed
    const long long *stream;   // stream index
    const long long *w0;       // windows the stream had completed before the push
    const long long *pc0;      // shared positions computed before the push (shared path; else 0)
    const long long *np;       // shared positions this push computes (shared path; else 0)
    const long long *rbase;    // [n_act + 1] prefix: staged frames (new positions, then frame 0 of each new window) of the entries before
    const long long *wbase;    // [n_act + 1] prefix: windows of the entries before
};

// where the samples of entry a's stream are: position p < n0 in ring[p % cap], p >= n0 at pcm[cidx + p]
struct SlideLiveSrc {
    const int16_t *ring, *pcm;
    long long n0, cidx;
    int cap;
};
__device__ __forceinline__ SlideLiveSrc slide_live_src(const int16_t *__restrict__ pcm, const int16_t *__restrict__ carry, const KwsSlideLiveMeta &m, int a,
                                                       int cap)
{
    SlideLiveSrc s;
    s.ring = carry + (size_t)m.stream[a] * cap;
    s.pcm = pcm;
    s.n0 = m.n0[a];
    s.cidx = m.off[a] - s.n0;
    s.cap = cap;
    return s;
}
// one sample (the predecessor of a frame: once per frame, one thread)
__device__ __forceinline__ int16_t slide_live_sample(const SlideLiveSrc &s, long long p)
{
    return p < s.n0 ? s.ring[p % s.cap] : s.pcm[s.cidx + p];
}

// the stream's samples [p0, p0 + n) (all of them below the stream's new end, n <= cap) to dst, dword-wide where both sides allow it.
// All threads of the block.
__device__ __forceinline__ void slide_live_copy(const SlideLiveSrc &s, long long p0, int n, int16_t *__restrict__ dst)
{
    const int tid = threadIdx.x, nt = blockDim.x;
    const long long left = s.n0 - p0;
    const int r = left <= 0 ? 0 : left >= n ? n : (int)left;         // the first r samples lie in the ring
    const int s0 = r > 0 ? (int)(p0 % s.cap) : 0;
    const int cap = s.cap;
    const int16_t *ring = s.ring;
    const long long c0 = s.cidx + p0;                                // sample i >= r: pcm[c0 + i]
    auto one = [&](int i) -> uint32_t {
        if (i >= r) return (uint16_t)s.pcm[c0 + i];
        int a = s0 + i;
        if (a >= cap) a -= cap;
        return (uint16_t)ring[a];
    };
    if ((((uintptr_t)dst) & 3) != 0) {                               // (windows of an odd length, staged back to back)
        for (int i = tid; i < n; i += nt) dst[i] = (int16_t)one(i);
        return;
    }
    uint32_t *d2 = (uint32_t *)dst;
    for (int i = tid; i < (n >> 1); i += nt) {
        const int e = 2 * i;
        uint32_t v;
        if (e >= r) {
            const int16_t *q = s.pcm + (c0 + e);
            v = (((uintptr_t)q) & 3) == 0 ? *(const uint32_t *)q : (uint32_t)(uint16_t)q[0] | ((uint32_t)(uint16_t)q[1] << 16);
        } else if (e + 1 < r) {
            int a = s0 + e;
            if (a >= cap) a -= cap;
            const int16_t *q = ring + a;
            if (a + 1 < cap && (((uintptr_t)q) & 3) == 0) v = *(const uint32_t *)q;
            else v = (uint32_t)(uint16_t)q[0] | ((uint32_t)(uint16_t)ring[a + 1 < cap ? a + 1 : 0] << 16);
        } else {
            v = one(e) | (one(e + 1) << 16);
        }
        d2[i] = v;
    }
    if ((n & 1) && tid == 0) dst[n - 1] = (int16_t)one(n - 1);
}

// Item item0 + m holds the push's staged frames (item0 + m) nfi + k, k < nfi (frames past n_frames: zeros).  Frame g belongs to the entry a
// with rbase[a] <= g < rbase[a + 1]; its first np[a] frames are the shared positions pc0[a] .. (at sample (j + pre) stride of the stream,
// predecessor the sample before), the others frame 0 of its new windows w0[a] .. (at sample w hop, predecessor sample w hop + clip - 1).
// pre = 0 (MFE block): no pre-emphasis, every predecessor is 0 and there is no per-window frame.  One block per item.
__global__ void kws_slide_live_stage_rows_kernel(const int16_t *__restrict__ pcm, const int16_t *__restrict__ carry, KwsSlideLiveMeta m, int n_act,
                                                 long long item0, int n_items, long long n_frames, int nfi, int S1, int used, int stride, long long hop,
                                                 int clip, int pre, int16_t *__restrict__ stage, float *__restrict__ wrap)
{
    for (int j = blockIdx.x; j < n_items; j += gridDim.x) {
        int16_t *item = stage + (size_t)j * nfi * S1;
        // frame k of the item: its entry (-1: no such frame), its first sample and its predecessor's position in the stream
        auto frame_of = [&](int k, long long *start, long long *pred) -> int {
            const long long g = (item0 + j) * nfi + k;
            if (k >= nfi || g >= n_frames) return -1;
            const int a = kws_prefix_owner(m.rbase, n_act, g);
            const long long i = g - m.rbase[a];
            if (i < m.np[a]) {
                *start = (m.pc0[a] + i + pre) * stride;
                *pred = *start - 1;
            } else {
                *start = (m.w0[a] + (i - m.np[a])) * hop;
                *pred = *start + clip - 1;
            }
            return a;
        };
        long long p = 0, q = 0;
        int a = frame_of(0, &p, &q);
        if (threadIdx.x == 0)
            wrap[j] = a >= 0 && pre ? (float)slide_live_sample(slide_live_src(pcm, carry, m, a, clip), q) * (1.0f / 32768.0f) : 0.0f;
        for (int k = 0; k < nfi; k++) {
            int16_t *dst = item + (size_t)k * S1;
            // a frame lies inside a completed window: every sample of it has arrived
            if (a >= 0) slide_live_copy(slide_live_src(pcm, carry, m, a, clip), p, used, dst);
            for (int i = (a >= 0 ? used : 0) + threadIdx.x; i < S1 - 1; i += blockDim.x) dst[i] = 0;
            a = frame_of(k + 1, &p, &q);
            if (threadIdx.x == 0) dst[S1 - 1] = a >= 0 && pre ? slide_live_sample(slide_live_src(pcm, carry, m, a, clip), q) : (int16_t)0;
        }
    }
}

// Window win0 + j of the push as clip j of `stage`: the entry's window w0 + (its place among the entry's windows), samples [w hop, + clip).
// One block per window.
__global__ void kws_slide_live_stage_clips_kernel(const int16_t *__restrict__ pcm, const int16_t *__restrict__ carry, KwsSlideLiveMeta m, int n_act,
                                                  long long win0, int n_win, long long hop, int clip, int16_t *__restrict__ stage)
{
    for (int j = blockIdx.x; j < n_win; j += gridDim.x) {
        const long long g = win0 + j;
        const int a = kws_prefix_owner(m.wbase, n_act, g);
        const long long w = m.w0[a] + (g - m.wbase[a]);
        slide_live_copy(slide_live_src(pcm, carry, m, a, clip), w * hop, clip, stage + (size_t)j * clip);
    }
}

// One block per window of the chunk.  Window w of entry a: row 0 (pre = 1) is the entry's staged frame np + (w - w0); row f >= pre is the
// shared position j = w hs + f - pre: below pc0 in the stream's ring (slot j % run), else the entry's staged frame j - pc0.
__global__ void kws_slide_live_gather_kernel(const float *__restrict__ rows, const float *__restrict__ kept, KwsSlideLiveMeta m, int n_act, long long win0,
                                             int n_win, long long hs, int run, int pre, int ncols, float *__restrict__ out)
{
    const int n_first = pre * ncols, n_rest = run * ncols;
    for (int jw = blockIdx.x; jw < n_win; jw += gridDim.x) {
        const long long g = win0 + jw;
        const int a = kws_prefix_owner(m.wbase, n_act, g);
        const long long i_w = g - m.wbase[a], j0 = (m.w0[a] + i_w) * hs, pc0 = m.pc0[a];
        const long long old = pc0 - j0;
        const int n_old = old <= 0 ? 0 : old >= run ? run : (int)old;              // the window's first n_old shared rows are retained ones
        const int slot0 = n_old > 0 ? (int)(j0 % run) : 0;
        const float *ring = kept + (size_t)m.stream[a] * run * ncols;
        const long long fresh = (m.rbase[a] + (j0 - pc0)) * ncols;                // row i >= n_old: rows + fresh + i ncols
        float *dst = out + (size_t)jw * (n_first + n_rest);
        for (int e = threadIdx.x; e < n_rest; e += blockDim.x) {
            const int i = e / ncols;
            float v;
            if (i < n_old) {
                int slot = slot0 + i;
                if (slot >= run) slot -= run;
                v = ring[slot * ncols + (e - i * ncols)];
            } else {
                v = rows[fresh + e];
            }
            dst[n_first + e] = v;
        }
        if (threadIdx.x < n_first) dst[threadIdx.x] = rows[(size_t)(m.rbase[a] + m.np[a] + i_w) * ncols + threadIdx.x];
    }
}

// One block per entry, after every stage and gather launch of the push (they read the slots this overwrites).  The stream keeps the samples
// from its next incomplete window's start on: the pushed ones among them, [max(n0, w1 hop), n1), go to their ring slots (fewer than cap: a
// push longer than the ring writes only what survives it).  run > 0 (shared path): the last min(np, run) positions the push computed go to
// their ring slots -- the slots of positions older than the last `run`, which no later window reads.
__global__ void kws_slide_live_commit_kernel(const int16_t *__restrict__ pcm, const float *__restrict__ rows, KwsSlideLiveMeta m, int n_act, long long hop,
                                             int cap, int run, int ncols, int16_t *__restrict__ carry, float *__restrict__ kept)
{
    const int tid = threadIdx.x, nt = blockDim.x;
    for (int a = blockIdx.x; a < n_act; a += gridDim.x) {
        const long long n0 = m.n0[a], n1 = n0 + m.len[a];
        const long long w1 = m.w0[a] + (m.wbase[a + 1] - m.wbase[a]);
        const long long c0 = w1 * hop > n0 ? w1 * hop : n0;
        if (c0 < n1) {
            const int cnt = (int)(n1 - c0), slot0 = (int)(c0 % cap);
            int16_t *ring = carry + (size_t)m.stream[a] * cap;
            const int16_t *src = pcm + (m.off[a] - n0 + c0);
            if (!(cap & 1) && (((uintptr_t)ring) & 3) == 0 && (((((uintptr_t)src) >> 1) ^ (uintptr_t)slot0) & 1) == 0) {
                // source and slot are dword-aligned together (an even ring: pairs never straddle its end)
                const int head = slot0 & 1, pairs = (cnt - head) >> 1;
                if (tid == 0 && head) ring[slot0] = src[0];
                for (int i = tid; i < pairs; i += nt) {
                    const int e = head + 2 * i;
                    int slot = slot0 + e;
                    if (slot >= cap) slot -= cap;
                    *(uint32_t *)(ring + slot) = *(const uint32_t *)(src + e);
                }
                if (tid == 0 && ((cnt - head) & 1)) {
                    int slot = slot0 + cnt - 1;
                    if (slot >= cap) slot -= cap;
                    ring[slot] = src[cnt - 1];
                }
            } else {
                for (int i = tid; i < cnt; i += nt) {
                    int slot = slot0 + i;
                    if (slot >= cap) slot -= cap;
                    ring[slot] = src[i];
                }
            }
        }
        const long long np = m.np[a];
        if (run <= 0 || np <= 0) continue;
        const int cnt = np < run ? (int)np : run;
        const long long r0 = m.pc0[a] + np - cnt;                   // the first position written
        const int slot0 = (int)(r0 % run);
        const float *src = rows + (size_t)(m.rbase[a] + (np - cnt)) * ncols;
        float *dst = kept + (size_t)m.stream[a] * run * ncols;
        for (int e = tid; e < cnt * ncols; e += nt) {
            const int i = e / ncols;
            int slot = slot0 + i;
            if (slot >= run) slot -= run;
            dst[slot * ncols + (e - i * ncols)] = src[e];
        }
    }
}

static KwsSlideLiveMeta slide_live_meta(const long long *d, int n_act)
{
    KwsSlideLiveMeta m;
    m.off = d; m.n0 = d + n_act; m.len = d + 2 * n_act; m.stream = d + 3 * n_act; m.w0 = d + 4 * n_act; m.pc0 = d + 5 * n_act; m.np = d + 6 * n_act;
    m.rbase = d + 7 * n_act; m.wbase = m.rbase + n_act + 1;
    return m;
}

int kws_launch_slide_live_stage_rows(const int16_t *pcm, const int16_t *carry, const long long *meta, int n_act, long long item0, int n_items,
                                     long long n_frames, int nfi, int S1, int used, int stride, long long hop, int clip, int pre, int16_t *stage,
                                     float *wrap, hipStream_t stream)
{
    (void)hipGetLastError();
    if (n_items <= 0) return 0;
    hipLaunchKernelGGL(kws_slide_live_stage_rows_kernel, dim3(n_items < 65536 ? n_items : 65536), dim3(256), 0, stream, pcm, carry,
                       slide_live_meta(meta, n_act), n_act, item0, n_items, n_frames, nfi, S1, used, stride, hop, clip, pre, stage, wrap);
    return (int)hipGetLastError();
}

int kws_launch_slide_live_stage_clips(const int16_t *pcm, const int16_t *carry, const long long *meta, int n_act, long long win0, int n_win, long long hop,
                                      int clip, int16_t *stage, hipStream_t stream)
{
    (void)hipGetLastError();
    if (n_win <= 0) return 0;
    hipLaunchKernelGGL(kws_slide_live_stage_clips_kernel, dim3(n_win < 65536 ? n_win : 65536), dim3(256), 0, stream, pcm, carry,
                       slide_live_meta(meta, n_act), n_act, win0, n_win, hop, clip, stage);
    return (int)hipGetLastError();
}

int kws_launch_slide_live_gather(const float *rows, const float *kept, const long long *meta, int n_act, long long win0, int n_win, long long hs, int run,
                                 int pre, int ncols, float *out, hipStream_t stream)
{
    (void)hipGetLastError();
    if (n_win <= 0) return 0;
    hipLaunchKernelGGL(kws_slide_live_gather_kernel, dim3(n_win < 65536 ? n_win : 65536), dim3(256), 0, stream, rows, kept, slide_live_meta(meta, n_act),
                       n_act, win0, n_win, hs, run, pre, ncols, out);
    return (int)hipGetLastError();
}

int kws_launch_slide_live_commit(const int16_t *pcm, const float *rows, const long long *meta, int n_act, long long hop, int cap, int run, int ncols,
                                 int16_t *carry, float *kept, hipStream_t stream)
{
    (void)hipGetLastError();
    if (n_act <= 0) return 0;
    hipLaunchKernelGGL(kws_slide_live_commit_kernel, dim3(n_act < 65536 ? n_act : 65536), dim3(256), 0, stream, pcm, rows, slide_live_meta(meta, n_act),
                       n_act, hop, cap, run, ncols, carry, kept);
    return (int)hipGetLastError();
}
