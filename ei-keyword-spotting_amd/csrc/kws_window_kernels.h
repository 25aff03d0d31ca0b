// kws_window_kernels.h -- device code shared by the kernel units of the four window pipelines (kws_scan_kernels.hip, kws_live_kernels.hip,
// kws_slide_kernels.hip, kws_slide_live_kernels.hip) and by the bank's (kws_bank_windows_kernels.hip).
#pragma once

// index a of the last prefix entry <= g (prefix[0] = 0, ascending, n entries + the total at prefix[n]): the recording, entry or slot that
// owns item g, empty ones skipped
__device__ __forceinline__ int kws_prefix_owner(const long long *__restrict__ prefix, int n, long long g)
{
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (prefix[mid] <= g) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// The per-entry tables of one push, n_act entries (the entries of the call that have work), each a device array:
struct KwsLiveMeta {
    const long long *off;      // the entry's chunk: pcm + off
    const long long *n0;       // samples the stream had before the push
    const long long *len;      // samples pushed
    const long long *stream;   // stream index
    const long long *k0, *k1;  // finished slices before / after the push
    const long long *fin;      // 1: the push finishes the stream (its state is not committed)
    const long long *fbase;    // [n_act + 1] prefix: slice-0 items of the entries before
    const long long *ibase;    // [n_act + 1] prefix: slice k >= 1 items of the entries before
    const long long *wbase;    // [n_act + 1] prefix: windows of the entries before
};

// the tables as kws_live.cpp packs them into one device array (kws_upload_tables)
static inline KwsLiveMeta live_meta(const long long *d, int n_act)
{
    KwsLiveMeta m;
    m.off = d; m.n0 = d + n_act; m.len = d + 2 * n_act; m.stream = d + 3 * n_act; m.k0 = d + 4 * n_act; m.k1 = d + 5 * n_act; m.fin = d + 6 * n_act;
    m.fbase = d + 7 * n_act; m.ibase = m.fbase + n_act + 1; m.wbase = m.ibase + n_act + 1;
    return m;
}
