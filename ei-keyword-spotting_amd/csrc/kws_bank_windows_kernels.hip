// kws_bank_windows_kernels.hip -- the moving average of the banks' window pipelines (kws_bank_windows.cpp): continuous mode's filter for
// every member of a bank in ONE launch.  One body, bank_maf<LIVE, ROUTED>: run_moving_average_filter (ei_run_classifier.h:134-145) per
// (member, recording or entry, label), one thread each; four kernels are its forms, each with the argument list its form needs:
//   kws_bank_maf_kernel<false>        scan: a fresh filter per recording over its windows in order -- kws_scan_maf_kernel for every member
//   kws_bank_maf_kernel<true>         live: the filter resumed from HBM and stored back, not stored for a stream the push finishes --
//                                     kws_live_maf_kernel for every member, with its w0 / k_full rule and its index as the window count mod taps
//   kws_bank_maf_routed_kernel        live, for a routed session: (entry, member) pairs the entry's route leaves out are skipped
//   kws_bank_maf_scan_routed_kernel   scan, for a routed call: (recording, member) pairs the recording's route leaves out are skipped
// The members' label counts differ, so a thread finds its member by walking the by-value table (at most KWS_BANK_MAX entries); member i's
// rows are [windows][labels[i]] in its own buffers.  The arithmetic is the two single-model kernels', operation for operation and in their
// order (subtract the oldest tap from the running sum, add the new value, store it as the tap, out = sum / (float)taps), so a member's rows
// are the bits its own call writes.  Each form compiles to the code it had as a kernel with a body of its own (profiles/bank_route_codeobj.md).
#include "kws_device.h"
#include "kws_window_kernels.h"
#include "kws_bank.h"

#include "../../include/kws/ei_compat.h"

#define KWS_BANK_TAPS (EI_CLASSIFIER_SLICES_PER_MODEL_WINDOW >> 1)

// thread t = a * total + r: recording / entry a, and the r-th (member, label) pair in table order (total = the members' labels summed).
// m: the push's per-entry tables; the scan form reads only its window prefix m.wbase [n + 1].  maf: the live form's filter states, member
// slot i's at maf + M.base[i] as [S][labels][taps + 1] (taps buf[j], then the running sum).  ROUTED: R.routes holds the route of every
// stream (live: [S]) or of every recording that has windows, in the order of wbase (scan: [n]), and R.member[i] the bank member behind
// slot i; a pair the route leaves out ends before it reads a row or its filter state.
template <bool LIVE, bool ROUTED>
__device__ __forceinline__ void bank_maf(const KwsBankMaf &M, const KwsBankMafRoute &R, const KwsLiveMeta &m, int n, int total, int k_full, float *__restrict__ maf)
{
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (long long)n * total) return;
    const int a = (int)(t / total);
    int l = (int)(t - (long long)a * total), i = 0;
    while (i < M.n - 1 && l >= M.labels[i]) { l -= M.labels[i]; ++i; }
    if (ROUTED && !((R.routes[LIVE ? m.stream[a] : a] >> R.member[i]) & 1u)) return;
    const int labels = M.labels[i];
    const float *raw = M.raw[i];
    float *scores = M.scores[i];
    const long long g0 = m.wbase[a], g1 = m.wbase[a + 1];
    long long w0 = 0;
    float *st = nullptr;
    bool store = false;
    if (LIVE) {
        if (g0 == g1) return;
        w0 = m.k0[a] > k_full ? m.k0[a] - k_full : 0;
        st = maf + M.base[i] + ((size_t)m.stream[a] * labels + l) * (KWS_BANK_TAPS + 1);
        store = !m.fin[a];
    }
    float buf[KWS_BANK_TAPS];
    float rs = 0.0f;
#pragma unroll
    for (int j = 0; j < KWS_BANK_TAPS; ++j) buf[j] = w0 ? st[j] : 0.0f;
    if (w0) rs = st[KWS_BANK_TAPS];
    int idx = (int)(w0 % KWS_BANK_TAPS);
    for (long long g = g0; g < g1; ++g) {
        const float v = raw[(size_t)g * labels + l];
        rs -= buf[idx];
        rs += v;
        buf[idx] = v;
        scores[(size_t)g * labels + l] = rs / (float)KWS_BANK_TAPS;
        if (++idx >= KWS_BANK_TAPS) idx = 0;
    }
    if (!store) return;
#pragma unroll
    for (int j = 0; j < KWS_BANK_TAPS; ++j) st[j] = buf[j];
    st[KWS_BANK_TAPS] = rs;
}

template <bool LIVE>
__global__ __launch_bounds__(64) void kws_bank_maf_kernel(KwsBankMaf M, KwsLiveMeta m, int n, int total, int k_full, float *__restrict__ maf)
{
    bank_maf<LIVE, false>(M, KwsBankMafRoute{}, m, n, total, k_full, maf);
}

__global__ __launch_bounds__(64) void kws_bank_maf_routed_kernel(KwsBankMaf M, KwsBankMafRoute R, KwsLiveMeta m, int n, int total, int k_full, float *__restrict__ maf)
{
    bank_maf<true, true>(M, R, m, n, total, k_full, maf);
}

__global__ __launch_bounds__(64) void kws_bank_maf_scan_routed_kernel(KwsBankMaf M, KwsBankMafRoute R, const long long *__restrict__ wbase, int n, int total)
{
    KwsLiveMeta m{};
    m.wbase = wbase;
    bank_maf<false, true>(M, R, m, n, total, 0, nullptr);
}

// What every launch starts with: one thread per (recording or entry, member, label) in blocks of 64; *total = the members' labels summed.
// 0: nothing to launch.
static unsigned bank_maf_blocks(const KwsBankMaf &M, int n_entries, int *total)
{
    (void)hipGetLastError();
    *total = 0;
    for (int i = 0; i < M.n; ++i) *total += M.labels[i];
    const long long n = (long long)n_entries * *total;
    return n <= 0 ? 0u : (unsigned)((n + 63) / 64);
}

int kws_launch_bank_maf_scan(const KwsBankMaf &M, const KwsBankMafRoute *R, const long long *wbase, int n_rec, hipStream_t stream)
{
    int total;
    const unsigned blocks = bank_maf_blocks(M, n_rec, &total);
    if (!blocks) return 0;
    KwsLiveMeta m{};
    m.wbase = wbase;
    if (R) hipLaunchKernelGGL(kws_bank_maf_scan_routed_kernel, dim3(blocks), dim3(64), 0, stream, M, *R, wbase, n_rec, total);
    else hipLaunchKernelGGL(kws_bank_maf_kernel<false>, dim3(blocks), dim3(64), 0, stream, M, m, n_rec, total, 0, (float *)nullptr);
    return (int)hipGetLastError();
}

int kws_launch_bank_maf_live(const KwsBankMaf &M, const KwsBankMafRoute *R, const long long *meta, int n_act, int k_full, float *maf, hipStream_t stream)
{
    int total;
    const unsigned blocks = bank_maf_blocks(M, n_act, &total);
    if (!blocks) return 0;
    if (R) hipLaunchKernelGGL(kws_bank_maf_routed_kernel, dim3(blocks), dim3(64), 0, stream, M, *R, live_meta(meta, n_act), n_act, total, k_full, maf);
    else hipLaunchKernelGGL(kws_bank_maf_kernel<true>, dim3(blocks), dim3(64), 0, stream, M, live_meta(meta, n_act), n_act, total, k_full, maf);
    return (int)hipGetLastError();
}
