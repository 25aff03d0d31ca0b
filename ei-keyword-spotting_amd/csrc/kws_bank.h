// kws_bank.h -- what the bank's units share (internal to libkws_mi355x.so): kws_bank.cpp and kws_bank_kernels.hip, and the bank forms of the
// window pipelines, kws_bank_windows.cpp and kws_bank_windows_kernels.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kws_plan.h"

#define KWS_BANK_MAX 16            // members of a bank (include/kws/kws.h)

// One record per member, in HBM for the bank's lifetime (written once by kws_bank_create): what the bank kernels need of an int8 member.
struct KwsBankRec {
    KwsNnPlan N;
    float in_scale;                // input tensor quantisation (N's own, next to the plan for the quantise-on-load)
    int in_zp;
};

// What changes from call to call travels in the launch arguments, so that no call writes the records: the members one launch serves
// (slot = blockIdx.y) and where their scores go.
struct KwsBankOut {
    int n;
    int rec[KWS_BANK_MAX];         // slot -> record
    float *scores[KWS_BANK_MAX];   // slot -> [n_clips][fc_out]
};

struct KwsBankQuant {
    int n;
    int zp[KWS_BANK_MAX];
    float scale[KWS_BANK_MAX];
    int8_t *q[KWS_BANK_MAX];       // [n] each
};

// Routed calls (a route per row: bit k set = member k scores it): slot i of a launch walks its member's list of rows instead of every row.
// A list is the `sel` list of the members' own launchers (kws_device.h): [0] = how many, [1 + j] = row, ascending; device memory, uploaded
// with the call.  A member with an empty list gets no slot.
struct KwsBankLists {
    const int *list[KWS_BANK_MAX];
};
// lists == NULL: the unrouted kernels over rows 0 .. n_rows - 1.  Otherwise the routed kernels, n_rows being the longest list of the launch
// (it sizes the grid).  row_len: values per feature row; routed, member slot j's tensor is written only at its listed rows.
int kws_launch_bank_nn_mfma(const KwsBankRec *recs, const KwsBankOut &out, const KwsBankLists *lists, int cp, const float *features, int n_rows, int grid_cap,
                            hipStream_t stream);
int kws_launch_bank_quantize(const float *features, int n_rows, int row_len, const KwsBankQuant &Q, const KwsBankLists *lists, hipStream_t stream);

// One moving-average launch for every member of a continuous-mode bank call (kws_bank_windows_kernels.hip): member slot i filters
// raw[i] [windows][labels[i]] into scores[i] (may be the same buffer); a live push keeps member i's filters at maf + base[i], stream after
// stream, [S][labels[i]][taps + 1].  By value in the launch arguments, as KwsBankOut.
struct KwsBankMaf {
    int n;
    int labels[KWS_BANK_MAX];
    const float *raw[KWS_BANK_MAX];
    float *scores[KWS_BANK_MAX];
    long long base[KWS_BANK_MAX];
};
// A routed call's moving average: routes (device) holds a route per stream (live: [S], every stream of the session) or per recording that
// has windows (scan: [n_rec], in the order of wbase), member[i] the bank member behind slot i; an (entry or recording, slot) pair whose
// route leaves the member out is skipped -- its rows and, live, its filter state are neither read nor written.
struct KwsBankMafRoute {
    const uint32_t *routes;
    int member[KWS_BANK_MAX];
};
// R == NULL: the unrouted kernel
int kws_launch_bank_maf_scan(const KwsBankMaf &M, const KwsBankMafRoute *R, const long long *wbase, int n_rec, hipStream_t stream);
int kws_launch_bank_maf_live(const KwsBankMaf &M, const KwsBankMafRoute *R, const long long *meta, int n_act, int k_full, float *maf, hipStream_t stream);

// ---- host side (kws_bank.cpp, kws_bank_windows.cpp: the units that include kws_internal.h first) ---------------------------------------------
#ifdef KWS_INTERNAL
#include <memory>

// A host vector that travels to the device with a call (one upload, behind the stream's earlier work): the upload reads the host copy
// when the stream gets there, so the copy is not rewritten before the previous upload has ended (wait), and it lives as long as the bank.
template <typename T>
struct BankUpload {
    std::vector<T> host;
    T *dev = nullptr;
    size_t cap = 0;
    hipEvent_t ev = nullptr;               // end of the latest upload
    bool ev_used = false;
    EI_IMPULSE_ERROR wait()
    {
        if (ev_used) HIP_TRY(hipEventSynchronize(ev));
        ev_used = false;
        return EI_IMPULSE_OK;
    }
    EI_IMPULSE_ERROR grow(size_t n) { return grow_buffer(&dev, &cap, n); }
    EI_IMPULSE_ERROR send(size_t n, hipStream_t s)
    {
        HIP_TRY(hipMemcpyAsync(dev, host.data(), n * sizeof(T), hipMemcpyHostToDevice, s));
        if (!ev) HIP_TRY(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
        HIP_TRY(hipEventRecord(ev, s));
        ev_used = true;
        return EI_IMPULSE_OK;
    }
    void release()
    {
        if (dev) (void)hipFree(dev);
        if (ev) (void)hipEventDestroy(ev);
    }
};

struct kws_bank {
    std::vector<kws_handle *> m;           // members, in the caller's order
    std::vector<kws_handle *> by_addr;     // the same, in the order their locks are taken
    int device = 0;
    KwsBankRec *d_rec = nullptr;           // [K] (int8 members' entries are filled)
    float *feat = nullptr;                 // the shared feature matrix of calls without `features`
    size_t feat_cap = 0;
    hipEvent_t ev = nullptr;               // end of the last call's work
    bool ev_used = false;
    BankUpload<int> lists;                 // a routed call's member lists, one chunk's at a time
    BankUpload<uint32_t> routes;           // a routed scan's routes, one per recording that has windows
    std::mutex mu;
};

// every member's lock in one order whatever the order of the members (two banks over the same handles cannot deadlock), and every
// member's scratch bracket: the call is a call on each of them (kws.h: streams and concurrency)
struct BankUse {
    std::unique_lock<std::mutex> own;
    std::vector<std::unique_lock<std::mutex>> locks;
    std::vector<std::unique_ptr<ScratchUse>> uses;        // released before the locks (declared after them)
    kws_bank *b;
    hipStream_t s;
    // skip_first: the pipeline runners bracket the first member themselves (kws_slide_run and the runners of kws_internal.h)
    // held: the bank's own lock, already taken by the caller (a push that reads the session's routes under it)
    BankUse(kws_bank *b_, hipStream_t s_, bool skip_first, std::unique_lock<std::mutex> &&held = std::unique_lock<std::mutex>()) : own(std::move(held)), b(b_), s(s_)
    {
        if (!own.owns_lock()) own = std::unique_lock<std::mutex>(b->mu);
        for (kws_handle *h : b->by_addr) locks.emplace_back(h->mu);
        for (size_t k = skip_first ? 1 : 0; k < b->m.size(); ++k) uses.emplace_back(new ScratchUse(b->m[k], s));
    }
    ~BankUse()
    {
        if (b->ev && hipEventRecord(b->ev, s) == hipSuccess) b->ev_used = true;
    }
};

// kws_bank.cpp.  bank_networks: every member's network from the feature matrix feat [B][F] (device); scores[k] + row0 * labels of member k
// is where its rows go.  routes: NULL (every member scores every row), or the routes of the B rows (host): member k then runs over the
// list of rows that name it.
KWS_INTERNAL EI_IMPULSE_ERROR bank_networks(kws_bank *b, const float *feat, size_t B, float *const *scores, size_t row0, hipStream_t s,
                                            const uint32_t *routes = nullptr);
// The K lists of n routes, packed: member k's at out[at[k]] as [count, rows ascending]; at[K] = the packed size.  One counting pass.
KWS_INTERNAL void kws_bank_route_lists(const uint32_t *routes, size_t n, size_t K, std::vector<int> &out, size_t *at);
// the first route of n that names a member >= K: its index, or n
KWS_INTERNAL size_t kws_bank_route_check(const uint32_t *routes, size_t n, size_t K);
// the refusal that follows from it ("<what> <index>: route ... names a member at or above the bank's ..."); routes == NULL: nothing to refuse
KWS_INTERNAL EI_IMPULSE_ERROR bank_routes_check(const kws_bank *b, const uint32_t *routes, size_t n, const char *what);
// The routes of a call's windows, in row order (kws_bank_windows.cpp): entry i has n_windows[i] windows, each with the route of its entry --
// route[index[i]] (a live push: the session's routes by stream), or route[i] where index is NULL (a recording call: the call's routes by
// recording).
KWS_INTERNAL void kws_bank_window_routes(const uint32_t *route, const size_t *index, const size_t *n_windows, size_t n, std::vector<uint32_t> &out);
// the membership rule: member k (handle h) has member 0's (a) device and front end, field by field; the refusal names the first that differs
KWS_INTERNAL EI_IMPULSE_ERROR bank_same_front_end(const kws_handle *a, const kws_handle *h, size_t k);
KWS_INTERNAL bool bank_wants_nothing(const kws_bank *b, float *const *scores, const float *features);
// where n feature rows of a call go: the caller's buffer, or (features == NULL) the bank's shared matrix, grown to hold them
KWS_INTERNAL EI_IMPULSE_ERROR bank_feature_rows(kws_bank *b, float *features, size_t n, float **f);
#endif
