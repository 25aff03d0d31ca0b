// kws_bank_windows.cpp -- the bank forms of the window pipelines (contract in include/kws/kws.h): recording scans and live streams in
// continuous mode, live one-shot windows and clips of their own lengths for K models that share one DSP block.
//   kws_bank_scan_recordings_device         kws_scan_run      (kws_scan.cpp); _routed_: a route per recording
//   kws_bank_slide_recordings_device        kws_slide_run     (kws_slide.cpp); _routed_: a route per recording
//   kws_bank_live_*                         kws_live_run      (kws_live.cpp), on a session of the first member opened without filter state
//   kws_bank_slide_live_*                   kws_slide_live_run (kws_slide_live.cpp), on a session of the first member
//   kws_bank_run_classifier_ragged_device   kws_ragged_run    (kws_ragged.cpp) with the network skipped
// Each is the first member's pipeline runner (kws_internal.h) with the bank's hooks: staging, the spectral kernels, gathering, carry and retained rows are the first member's and run ONCE; every chunk of
// gathered windows ends in bank_window_finish (cmvnw once, then every member's network: bank_networks of kws_bank.cpp), and continuous mode's
// moving average is ONE launch of kws_bank_maf_kernel for all members (kws_bank_windows_kernels.hip).  What is per member: its scores, its raw scores and,
// in a live session, its filters -- sum_k labels_k x (taps + 1) floats per stream, in one allocation of the session.
// These are the launches of KWS_MODE_EXACT: nothing here reads or writes a member's mode, fast counters or logits tap, and no hook of the
// bank's asks for the idle finishing call (finish_idle) that the single-model pushes use to reset their counters.
// A call that takes routes is the entry point; the call without is that call with routes = NULL, and a routed call's hooks are the unrouted
// call's over a context that also holds the routes.
#include "kws_internal.h"
#include "kws_bank.h"

#include "../../include/kws/ei_compat.h"

#include <algorithm>

static const int kBankTaps = EI_CLASSIFIER_SLICES_PER_MODEL_WINDOW >> 1;

static size_t bank_max_labels(const kws_bank *b)
{
    size_t c = 0;
    for (const kws_handle *h : b->m) c = std::max(c, h->model.labels.size());
    return c;
}

void kws_bank_window_routes(const uint32_t *route, const size_t *index, const size_t *n_windows, size_t n, std::vector<uint32_t> &out)
{
    out.clear();
    for (size_t i = 0; i < n; ++i) out.insert(out.end(), n_windows[i], route[index ? index[i] : i]);
}

// What the finishing step of a chunk of gathered windows needs.  A routed push or recording call adds the routes of its entries (route_by):
// a window's route is its stream's (a push: the session's routes, by streams[i]) or its recording's (a recording call: the call's routes,
// index == NULL).  Every entry's window count is on the host before a hook is called (a push: the runner has filled the caller's
// n_windows; a recording call: the pipeline's count per recording), so the per-window table is built at the first non-empty chunk, before
// anything of the networks is enqueued, and each chunk is handed its part.
struct BankWindows {
    kws_bank *b;
    float *const *scores;          // [K]: where member k's rows go (NULL: skipped)
    float *features;               // the caller's [windows][F], or NULL: the bank's shared matrix, a chunk at a time
    const uint32_t *routes = nullptr;      // [windows] (host), or NULL: every member scores every window
    const uint32_t *route = nullptr;       // the entries' routes [S] or [R], from which `routes` is built (NULL: `routes` is as given)
    const size_t *index = nullptr, *n_windows = nullptr;       // the entries' streams (NULL: entry i is recording i) and window counts
    size_t n = 0;
    std::vector<uint32_t> table;
    void route_by(const uint32_t *route_, const size_t *index_, const size_t *n_windows_, size_t n_) { route = route_; index = index_; n_windows = n_windows_; n = n_; }
};

// the finishing step of a chunk of gathered windows for a bank: cmvnw (the MFE normalisation) once through the first member, then every member
static EI_IMPULSE_ERROR bank_window_finish(void *ctx, float *win, size_t n, size_t g0, hipStream_t s)
{
    if (n == 0) return EI_IMPULSE_OK;
    BankWindows &c = *(BankWindows *)ctx;
    if (c.route && !c.routes) {
        kws_bank_window_routes(c.route, c.index, c.n_windows, c.n, c.table);
        c.routes = c.table.data();
    }
    float *f;
    EI_IMPULSE_ERROR e = bank_feature_rows(c.b, c.features ? c.features + g0 * c.b->m[0]->model.nn_input_frame_size : nullptr, n, &f);
    if (e) return e;
    if ((e = cmvn_nn_device(c.b->m[0], win, n, f, nullptr, nullptr, nullptr, nullptr, nullptr, s))) return e;
    return bank_networks(c.b, f, n, c.scores, g0, s, c.routes ? c.routes + g0 : nullptr);
}

// the ragged call's finishing step: the DSP route has written the full-stride feature rows; every member's network reads them
static EI_IMPULSE_ERROR bank_ragged_finish(void *ctx, float *f, size_t B, size_t, hipStream_t s)
{
    BankWindows &c = *(BankWindows *)ctx;
    return bank_networks(c.b, f, B, c.scores, 0, s, c.routes);
}

// Continuous mode for a bank: the chunks' raw scores go where each member's moving average reads them -- its raw_scores, or its scores
// (filtered in place) -- and the filter step is one launch over the members that are not skipped.
struct BankContinuous {
    BankWindows w;                         // (first: bank_window_finish reads it)
    float *raw[KWS_BANK_MAX];              // w.scores points here
    float *const *scores;
    int k_full;                            // the live form (maf != NULL): the layout's first window step
    float *maf;
    const long long *base;                 // [K] floats before member k's filters
    const uint32_t *d_routes = nullptr;    // a routed live push: the session's routes [S] in HBM (NULL: every pair is filtered)
    const std::vector<uint32_t> *scan_routes = nullptr;    // a routed scan: the routes of the recordings that have windows, in their order (host)
    uint32_t wanted = ~0u;                 // a routed scan: the members some recording with windows names; the others get no filter slot
    BankContinuous(kws_bank *b, float *const *scores_, float *const *raw_scores, int k_full_ = 0, float *maf_ = nullptr, const long long *base_ = nullptr)
        : w{ b, raw, nullptr }, scores(scores_), k_full(k_full_), maf(maf_), base(base_)
    {
        for (size_t k = 0; k < b->m.size(); ++k) raw[k] = !scores[k] ? nullptr : raw_scores && raw_scores[k] ? raw_scores[k] : scores[k];
    }
    BankContinuous(const BankContinuous &) = delete;       // (w.scores points into this object)
};
static EI_IMPULSE_ERROR bank_continuous_maf(void *ctx, const long long *meta, int n, hipStream_t s)
{
    BankContinuous &c = *(BankContinuous *)ctx;
    kws_bank *b = c.w.b;
    KwsBankMaf M{};
    KwsBankMafRoute R{};
    R.routes = c.d_routes;
    for (size_t k = 0; k < b->m.size(); ++k) {
        if (!c.scores[k] || !((c.wanted >> k) & 1u)) continue;
        R.member[M.n] = (int)k;
        M.labels[M.n] = (int)b->m[k]->model.labels.size();
        M.raw[M.n] = c.raw[k];
        M.scores[M.n] = c.scores[k];
        M.base[M.n] = c.base ? c.base[k] : 0;
        ++M.n;
    }
    if (c.scan_routes) {
        // the routes travel with the call, behind the stream's earlier work
        if (M.n == 0) return EI_IMPULSE_OK;
        if ((size_t)n != c.scan_routes->size()) return fail(KWS_ERROR_BAD_ARGUMENT, "routed scan: %d recordings with windows, %zu routes", n, c.scan_routes->size());
        EI_IMPULSE_ERROR e = b->routes.wait();
        if (e) return e;
        b->routes.host = *c.scan_routes;
        if ((e = b->routes.grow((size_t)n)) || (e = b->routes.send((size_t)n, s))) return e;
        R.routes = b->routes.dev;
    }
    const KwsBankMafRoute *routed = R.routes ? &R : nullptr;
    const int rc = c.maf ? kws_launch_bank_maf_live(M, routed, meta, n, c.k_full, c.maf, s) : kws_launch_bank_maf_scan(M, routed, meta, n, s);
    if (routed) KWS_LAUNCH_TRY("routed bank moving-average kernel", rc);
    else KWS_LAUNCH_TRY("bank moving-average kernel", rc);
    return EI_IMPULSE_OK;
}

// the session's routes: every stream to every member until kws_bank_*_route says otherwise
struct BankRoutes {
    std::vector<uint32_t> route;           // [S]
    uint32_t every = 0;
    bool routed = false;                   // some stream's route is not `every`
    void open(size_t S, size_t K) { every = (1u << K) - 1u; route.assign(S, every); }
    // the checks of kws_bank_*_route; the first offending entry is named
    EI_IMPULSE_ERROR check(const size_t *streams, size_t n, const uint32_t *routes, size_t K) const
    {
        if (n > 0 && (!streams || !routes)) return fail(KWS_ERROR_BAD_ARGUMENT, "null argument");
        for (size_t i = 0; i < n; ++i) {
            if (streams[i] >= route.size()) return fail(KWS_ERROR_BAD_ARGUMENT, "entry %zu: stream %zu of %zu", i, streams[i], route.size());
            if (routes[i] >> K) return fail(KWS_ERROR_BAD_ARGUMENT, "entry %zu: route 0x%x names a member at or above the bank's %zu", i, routes[i], K);
        }
        return EI_IMPULSE_OK;
    }
    void set(const size_t *streams, size_t n, const uint32_t *routes)
    {
        for (size_t i = 0; i < n; ++i) route[streams[i]] = routes[i];
        routed = false;
        for (uint32_t r : route) routed = routed || r != every;
    }
};

// (the sessions: the bank, the first member's session -- carry, retained rows, mirrors, per-push scratch: ONE copy -- and what is per member)
struct kws_bank_live {
    kws_bank *b = nullptr;
    kws_live *core = nullptr;
    ScanLayout L;
    float *maf = nullptr;                  // state in HBM: member k's [S][labels_k][taps + 1] at base[k]
    std::vector<long long> base;
    BankRoutes routes;
    uint32_t *d_routes = nullptr;          // the routes in HBM, where the routed moving average reads them (allocated by the first kws_bank_live_route)
    std::vector<char> pushed;              // [S]: the stream has been pushed to since its start (create, reset or finish): its route is fixed
};
struct kws_bank_slide_live {
    kws_bank *b = nullptr;
    kws_slide_live *core = nullptr;
    BankRoutes routes;
};

// the end of the bank's latest call, this session's last push included (BankUse records it), before a session's memory goes
static void bank_wait(kws_bank *b)
{
    (void)hipSetDevice(b->device);
    if (b->ev && b->ev_used) (void)hipEventSynchronize(b->ev);
}

extern "C" {
#pragma GCC visibility push(default)

// A recording call's routes: every recording's window count and, of the recordings that have windows, their routes in order and the members
// they name.  every: the recordings that have windows all name every member (the unrouted call).
struct BankRecordingRoutes {
    std::vector<size_t> n_windows;         // [R]
    std::vector<uint32_t> active;
    uint32_t wanted = 0;
    bool every = true;
    void add(uint32_t route, size_t W, size_t K)
    {
        n_windows.push_back(W);
        if (!W) return;
        active.push_back(route);
        wanted |= route;
        every = every && route == (1u << K) - 1u;
    }
};

EI_IMPULSE_ERROR kws_bank_scan_recordings_device(kws_bank *b, const int16_t *pcm, const size_t *offsets, const size_t *lengths, size_t R,
                                                 size_t slice_samples, float *const *scores, float *const *raw_scores, void *stream)
{
    return kws_bank_scan_recordings_routed_device(b, pcm, offsets, lengths, R, nullptr, slice_samples, scores, raw_scores, stream);
}

EI_IMPULSE_ERROR kws_bank_scan_recordings_routed_device(kws_bank *b, const int16_t *pcm, const size_t *offsets, const size_t *lengths, size_t R,
                                                        const uint32_t *routes, size_t slice_samples, float *const *scores, float *const *raw_scores,
                                                        void *stream)
{
    if (!b || !scores) return fail(KWS_ERROR_BAD_ARGUMENT, "null argument");
    if (bank_wants_nothing(b, scores, nullptr)) return fail(KWS_ERROR_BAD_ARGUMENT, "no output requested: every scores[k] is NULL");
    BankRecordingRoutes rr;
    if (routes) {
        // (the routes are sorted out before the pipeline runs, so what it would refuse of the arguments read here is refused here)
        if (R > 0 && (!pcm || !offsets || !lengths)) return fail(KWS_ERROR_BAD_ARGUMENT, "null argument");
        if (R > 0x3fffffff) return fail(KWS_ERROR_BAD_ARGUMENT, "too many recordings");
        EI_IMPULSE_ERROR e = bank_routes_check(b, routes, R, "recording");
        if (e) return e;
        ScanLayout L;
        if ((e = scan_layout(b->m[0], slice_samples, &L))) return e;
        for (size_t r = 0; r < R; ++r) rr.add(routes[r], L.windows(lengths[r] / slice_samples), b->m.size());
    }
    HIP_TRY(hipSetDevice(b->device));
    hipStream_t s = (hipStream_t)stream;
    BankUse use(b, s, true);
    BankContinuous ctx(b, scores, raw_scores);
    if (!rr.every) {
        ctx.w.route_by(routes, nullptr, rr.n_windows.data(), R);
        ctx.scan_routes = &rr.active;
        ctx.wanted = rr.wanted;
    }
    return kws_scan_run(b->m[0], pcm, offsets, lengths, R, slice_samples, bank_max_labels(b), 0, bank_window_finish, bank_continuous_maf, &ctx, s);
}

EI_IMPULSE_ERROR kws_bank_slide_recordings_device(kws_bank *b, const int16_t *pcm, const size_t *offsets, const size_t *lengths, size_t R,
                                                  size_t hop_samples, int flags, float *const *scores, float *features, void *stream)
{
    return kws_bank_slide_recordings_routed_device(b, pcm, offsets, lengths, R, nullptr, hop_samples, flags, scores, features, stream);
}

EI_IMPULSE_ERROR kws_bank_slide_recordings_routed_device(kws_bank *b, const int16_t *pcm, const size_t *offsets, const size_t *lengths, size_t R,
                                                         const uint32_t *routes, size_t hop_samples, int flags, float *const *scores, float *features,
                                                         void *stream)
{
    if (!b || !scores) return fail(KWS_ERROR_BAD_ARGUMENT, "null argument");
    if (bank_wants_nothing(b, scores, features)) return fail(KWS_ERROR_BAD_ARGUMENT, "no output requested: every scores[k] and features are NULL");
    // the window count is any member's; the bound on windows x labels holds for the member with the most labels (a bad hop or flags, NULL
    // lengths, too many windows: any member's plan refuses them)
    kws_slide_plan_info I;
    EI_IMPULSE_ERROR e;
    for (kws_handle *h : b->m)
        if ((e = kws_slide_plan(h, lengths, R, hop_samples, flags, &I))) return e;
    if ((e = bank_routes_check(b, routes, R, "recording"))) return e;
    BankRecordingRoutes rr;
    for (size_t r = 0; routes && r < R; ++r) {
        size_t W = 0;
        if ((e = kws_slide_window_count(b->m[0], lengths[r], hop_samples, &W))) return e;
        rr.add(routes[r], W, b->m.size());
    }
    HIP_TRY(hipSetDevice(b->device));
    hipStream_t s = (hipStream_t)stream;
    BankUse use(b, s, true);
    BankWindows ctx{ b, scores, features };
    if (!rr.every) ctx.route_by(routes, nullptr, rr.n_windows.data(), R);
    return kws_slide_run(b->m[0], pcm, offsets, lengths, R, hop_samples, flags, 0, bank_window_finish, &ctx, s);
}

EI_IMPULSE_ERROR kws_bank_live_create(kws_bank *b, size_t S, size_t slice_samples, kws_bank_live **out)
{
    if (out) *out = nullptr;
    if (!b || !out) return fail(KWS_ERROR_BAD_ARGUMENT, "bad argument");
    std::unique_ptr<kws_bank_live> lv(new kws_bank_live());
    lv->b = b;
    EI_IMPULSE_ERROR e = kws_live_open(b->m[0], S, slice_samples, 0, &lv->core);
    if (e) return e;
    (void)scan_layout(b->m[0], slice_samples, &lv->L);             // (kws_live_open has accepted the slicing)
    lv->routes.open(S, b->m.size());
    lv->pushed.assign(S, 0);
    long long floats = 0;
    for (const kws_handle *h : b->m) {
        lv->base.push_back(floats);
        floats += (long long)(S * h->model.labels.size() * (kBankTaps + 1));
    }
    // (a stream's filters are read only once it has had a window; cleared so that no stale value can ever reach a result)
    if (hipMalloc((void **)&lv->maf, (size_t)floats * sizeof(float)) != hipSuccess || hipMemset(lv->maf, 0, (size_t)floats * sizeof(float)) != hipSuccess) {
        if (lv->maf) (void)hipFree(lv->maf);
        kws_live_destroy(lv->core);
        return fail(KWS_ERROR_HIP, "bank live session allocation failed");
    }
    *out = lv.release();
    return EI_IMPULSE_OK;
}

void kws_bank_live_destroy(kws_bank_live *lv)
{
    if (!lv) return;
    {
        std::lock_guard<std::mutex> lk(lv->b->mu);
        bank_wait(lv->b);
        kws_live_destroy(lv->core);
        if (lv->maf) (void)hipFree(lv->maf);
        if (lv->d_routes) (void)hipFree(lv->d_routes);
    }
    delete lv;
}

EI_IMPULSE_ERROR kws_bank_live_reset(kws_bank_live *lv, const size_t *streams, size_t n)
{
    if (!lv) return fail(KWS_ERROR_BAD_ARGUMENT, "null argument");
    std::lock_guard<std::mutex> lk(lv->b->mu);
    const EI_IMPULSE_ERROR e = kws_live_reset(lv->core, streams, n);
    if (e) return e;
    // (routes stay; the streams are in their reset state again, where a route may change)
    if (!streams) std::fill(lv->pushed.begin(), lv->pushed.end(), 0);
    else for (size_t i = 0; i < n; ++i) lv->pushed[streams[i]] = 0;
    return EI_IMPULSE_OK;
}

EI_IMPULSE_ERROR kws_bank_live_route(kws_bank_live *lv, const size_t *streams, size_t n, const uint32_t *routes)
{
    if (!lv) return fail(KWS_ERROR_BAD_ARGUMENT, "null argument");
    kws_bank *b = lv->b;
    std::lock_guard<std::mutex> lk(b->mu);
    EI_IMPULSE_ERROR e = lv->routes.check(streams, n, routes, b->m.size());
    if (e) return e;
    // a member's moving-average filter must see every window of a stream it serves: no change once the stream has been pushed to
    for (size_t i = 0; i < n; ++i)
        if (lv->pushed[streams[i]])
            return fail(KWS_ERROR_BAD_ARGUMENT, "entry %zu: stream %zu has been pushed to; its route changes only after a reset", i, streams[i]);
    if (n == 0) return EI_IMPULSE_OK;
    HIP_TRY(hipSetDevice(b->device));
    const size_t S = lv->routes.route.size();
    if (!lv->d_routes) HIP_TRY(hipMalloc((void **)&lv->d_routes, S * sizeof(uint32_t)));
    // (a push enqueued earlier may still read the old table: the bank's event marks the end of its latest call)
    bank_wait(b);
    BankRoutes next = lv->routes;
    next.set(streams, n, routes);
    HIP_TRY(hipMemcpy(lv->d_routes, next.route.data(), S * sizeof(uint32_t), hipMemcpyHostToDevice));
    lv->routes = next;
    return EI_IMPULSE_OK;
}

EI_IMPULSE_ERROR kws_bank_live_window_count(const kws_bank_live *lv, size_t stream, size_t n_new, int finish, size_t *n_windows)
{
    if (!lv) return fail(KWS_ERROR_BAD_ARGUMENT, "null argument");
    std::lock_guard<std::mutex> lk(lv->b->mu);
    return kws_live_window_count(lv->core, stream, n_new, finish, n_windows);
}

EI_IMPULSE_ERROR kws_bank_live_push_device(kws_bank_live *lv, size_t n, const size_t *streams, const int16_t *pcm, const size_t *offsets,
                                           const size_t *lengths, const int *finish, float *const *scores, float *const *raw_scores,
                                           size_t *n_windows, void *stream)
{
    if (!lv) return fail(KWS_ERROR_BAD_ARGUMENT, "null argument");
    kws_bank *b = lv->b;
    // every member's filter must see every window of the streams it serves: a member is skipped only where no stream named in the push
    // routes to it (a session that was never routed: no member is skipped)
    std::unique_lock<std::mutex> own(b->mu);
    const bool routed = lv->routes.routed;
    uint32_t wanted = routed ? 0 : lv->routes.every;
    for (size_t i = 0; routed && streams && i < n; ++i)
        if (streams[i] < lv->routes.route.size()) wanted |= lv->routes.route[streams[i]];
    for (size_t k = 0; scores && k < b->m.size(); ++k)
        if (!scores[k] && ((wanted >> k) & 1u))
            return fail(KWS_ERROR_BAD_ARGUMENT, routed ? "scores[%zu] is NULL: a stream named in this push routes to that member" : "scores[%zu] is NULL: a live push skips no member", k);
    HIP_TRY(hipSetDevice(b->device));
    hipStream_t s = (hipStream_t)stream;
    BankUse use(b, s, true, std::move(own));
    float *const none[KWS_BANK_MAX] = { nullptr };
    BankContinuous ctx(b, scores ? scores : none, raw_scores, (int)lv->L.k_full, lv->maf, lv->base.data());
    if (routed) {
        ctx.d_routes = lv->d_routes;
        ctx.w.route_by(lv->routes.route.data(), streams, n_windows, n);
    }
    const EI_IMPULSE_ERROR e = kws_live_run(lv->core, n, streams, pcm, offsets, lengths, finish, scores, n_windows, bank_max_labels(b), 0, 0, bank_window_finish,
                                            bank_continuous_maf, &ctx, s);
    if (e) return e;
    // (a stream the push finished starts over: its route may change again)
    for (size_t i = 0; i < n; ++i) lv->pushed[streams[i]] = !(finish && finish[i]);
    return EI_IMPULSE_OK;
}

EI_IMPULSE_ERROR kws_bank_slide_live_create(kws_bank *b, size_t S, size_t hop_samples, int flags, kws_bank_slide_live **out)
{
    if (out) *out = nullptr;
    if (!b || !out) return fail(KWS_ERROR_BAD_ARGUMENT, "bad argument");
    std::unique_ptr<kws_bank_slide_live> sl(new kws_bank_slide_live());
    sl->b = b;
    EI_IMPULSE_ERROR e = kws_slide_live_create(b->m[0], S, hop_samples, flags, &sl->core);
    if (e) return e;
    sl->routes.open(S, b->m.size());
    *out = sl.release();
    return EI_IMPULSE_OK;
}

void kws_bank_slide_live_destroy(kws_bank_slide_live *sl)
{
    if (!sl) return;
    {
        std::lock_guard<std::mutex> lk(sl->b->mu);
        bank_wait(sl->b);
        kws_slide_live_destroy(sl->core);
    }
    delete sl;
}

int kws_bank_slide_live_path(const kws_bank_slide_live *sl) { return sl ? kws_slide_live_path(sl->core) : 0; }

EI_IMPULSE_ERROR kws_bank_slide_live_reset(kws_bank_slide_live *sl, const size_t *streams, size_t n)
{
    if (!sl) return fail(KWS_ERROR_BAD_ARGUMENT, "null argument");
    std::lock_guard<std::mutex> lk(sl->b->mu);
    return kws_slide_live_reset(sl->core, streams, n);
}

EI_IMPULSE_ERROR kws_bank_slide_live_route(kws_bank_slide_live *sl, const size_t *streams, size_t n, const uint32_t *routes)
{
    if (!sl) return fail(KWS_ERROR_BAD_ARGUMENT, "null argument");
    std::lock_guard<std::mutex> lk(sl->b->mu);
    const EI_IMPULSE_ERROR e = sl->routes.check(streams, n, routes, sl->b->m.size());
    if (e) return e;
    sl->routes.set(streams, n, routes);          // (no per-member state: a route may change between any two pushes)
    return EI_IMPULSE_OK;
}

EI_IMPULSE_ERROR kws_bank_slide_live_window_count(const kws_bank_slide_live *sl, size_t stream, size_t n_new, size_t *n_windows)
{
    if (!sl) return fail(KWS_ERROR_BAD_ARGUMENT, "null argument");
    std::lock_guard<std::mutex> lk(sl->b->mu);
    return kws_slide_live_window_count(sl->core, stream, n_new, n_windows);
}

EI_IMPULSE_ERROR kws_bank_slide_live_push_device(kws_bank_slide_live *sl, size_t n, const size_t *streams, const int16_t *pcm,
                                                 const size_t *offsets, const size_t *lengths, float *const *scores, float *features,
                                                 size_t *n_windows, void *stream)
{
    if (!sl) return fail(KWS_ERROR_BAD_ARGUMENT, "null argument");
    kws_bank *b = sl->b;
    if (scores && bank_wants_nothing(b, scores, features)) return fail(KWS_ERROR_BAD_ARGUMENT, "no output requested: every scores[k] and features are NULL");
    HIP_TRY(hipSetDevice(b->device));
    hipStream_t s = (hipStream_t)stream;
    BankUse use(b, s, true);
    BankWindows ctx{ b, scores, features };
    if (sl->routes.routed) ctx.route_by(sl->routes.route.data(), streams, n_windows, n);
    return kws_slide_live_run(sl->core, n, streams, pcm, offsets, lengths, scores, n_windows, bank_max_labels(b), 0, 0, bank_window_finish, &ctx, s);
}

EI_IMPULSE_ERROR kws_bank_run_classifier_ragged_device(kws_bank *b, const int16_t *pcm, const size_t *offsets, const size_t *lengths, size_t B,
                                                       float *const *scores, float *features, void *stream)
{
    return kws_bank_run_classifier_ragged_routed_device(b, pcm, offsets, lengths, B, nullptr, scores, features, stream);
}

EI_IMPULSE_ERROR kws_bank_run_classifier_ragged_routed_device(kws_bank *b, const int16_t *pcm, const size_t *offsets, const size_t *lengths, size_t B,
                                                              const uint32_t *routes, float *const *scores, float *features, void *stream)
{
    if (!b || !scores) return fail(KWS_ERROR_BAD_ARGUMENT, "null argument");
    if (bank_wants_nothing(b, scores, features)) return fail(KWS_ERROR_BAD_ARGUMENT, "no output requested: every scores[k] and features are NULL");
    if (B >= ((size_t)1 << 31)) return fail(KWS_ERROR_BAD_ARGUMENT, "batch too large");
    EI_IMPULSE_ERROR e = bank_routes_check(b, routes, B, "clip");
    if (e) return e;
    if (B == 0) return EI_IMPULSE_OK;
    HIP_TRY(hipSetDevice(b->device));
    hipStream_t s = (hipStream_t)stream;
    BankUse use(b, s, true);
    float *f;
    if ((e = bank_feature_rows(b, features, B, &f))) return e;
    BankWindows ctx{ b, scores, features, routes };
    return kws_ragged_run(b->m[0], pcm, offsets, lengths, B, f, nullptr, 0, 0, bank_ragged_finish, &ctx, s);
}

#pragma GCC visibility pop
}
