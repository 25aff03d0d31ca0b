// kws_window_kernels.h -- device code shared by the kernel units of the four window pipelines (kws_scan_kernels.hip, kws_live_kernels.hip,
// kws_slide_kernels.hip, kws_slide_live_kernels.hip).
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
