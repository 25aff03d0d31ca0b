// kws_pool.cpp -- pools: up to KWS_POOL_MAX int8 models of the two-block matrix-core shape behind one DSP block, ONE member per row
// (kws_pool_*; contract in include/kws/kws.h).  Where a bank serves any subset of sixteen members of any graph family per row, with
// outputs and filter state per member, a pool serves hundreds of tenants of the one family Edge Impulse hands everybody:
//   front end      ONCE, through the first member and with its own exact launches: mfcc_fused_device for clips, kws_ragged_run for clips of
//                  their own lengths, kws_live_run for live streams -- the runners of kws_internal.h, unchanged, with the pool's hooks
//   networks       ONE launch of kws_pool_nn_mfma_kernel whatever K (pool_networks): the rows' members become ascending row lists, the lists
//                  are cut into work items of at most KWS_POOL_ITEM_ROWS rows, and items and lists go up in one upload with the call
//   scores         ONE matrix [rows][stride], stride = the most labels any member has; row i gets its member's labels, nothing else is written
//   live sessions  one filter state [S][stride][taps + 1] and one moving-average launch per push (kws_pool_maf_live_kernel); the streams'
//                  members are the session's, on the host and in HBM
//   recordings     kws_scan_run and kws_slide_run with the same finishing hook: a window's member is its recording's; the scan's moving
//                  average is one launch of kws_pool_maf_scan_kernel, the members of the recordings that have windows going up with the call
//   one-shot live  kws_slide_live_run on a session of the first member; no state per member, so a stream's member is host data only
//   cepstra in     cmvn_nn_device once, then pool_networks
// A pool call is a call on the pool and on the FIRST member only: it takes that member's lock and scratch bracket and nobody else's -- of
// the other members it reads only the immutable device weights their records point to.  These are the launches of KWS_MODE_EXACT: nothing
// here reads or writes a member's mode, fast counters or logits tap.
#include "kws_internal.h"
#include "kws_pool.h"

#include "../../include/kws/ei_compat.h"

#include <algorithm>

static const int kPoolTaps = EI_CLASSIFIER_SLICES_PER_MODEL_WINDOW >> 1;

// rows per work item: KWS_POOL_ITEM_ROWS; the development build reads another value from the environment (tools/gpu_pool_rate.py measures the candidates)
static int pool_item_rows()
{
    const char *e = KWS_DEV_ENV("KWS_DEV_POOL_ITEM_ROWS");
    const int v = e ? atoi(e) : 0;
    return v > 0 ? v : KWS_POOL_ITEM_ROWS;
}

size_t kws_pool_items(const uint32_t *member, size_t n, size_t K, int item_rows, std::vector<int> &out, std::vector<int> &fill)
{
    fill.assign(K, 0);
    size_t named = 0, n_items = 0;
    for (size_t i = 0; i < n; ++i)
        if (member[i] != KWS_POOL_NONE) { ++fill[member[i]]; ++named; }
    for (size_t k = 0; k < K; ++k) n_items += (size_t)((fill[k] + item_rows - 1) / item_rows);
    out.resize(4 * n_items + named);
    size_t it = 0;
    int at = 0;
    for (size_t k = 0; k < K; ++k) {
        const int c = fill[k];
        for (int p = 0; p < c; p += item_rows, ++it) {
            out[4 * it] = (int)k; out[4 * it + 1] = at + p; out[4 * it + 2] = std::min(item_rows, c - p); out[4 * it + 3] = 0;
        }
        fill[k] = at;
        at += c;
    }
    int *rows = out.data() + 4 * n_items;
    for (size_t i = 0; i < n; ++i)
        if (member[i] != KWS_POOL_NONE) rows[fill[member[i]]++] = (int)i;
    return n_items;
}

size_t kws_pool_member_check(const uint32_t *member, size_t n, size_t K)
{
    for (size_t i = 0; i < n; ++i)
        if (member[i] >= K && member[i] != KWS_POOL_NONE) return i;
    return n;
}

void kws_pool_window_members(const uint32_t *assign, const size_t *index, const size_t *n_windows, size_t n, std::vector<uint32_t> &out)
{
    out.clear();
    for (size_t i = 0; i < n; ++i) out.insert(out.end(), n_windows[i], assign[index ? index[i] : i]);
}

// the refusal of a call whose rows name a member the pool does not have; what: the call's word for a row
static EI_IMPULSE_ERROR pool_members_check(const kws_pool *p, const uint32_t *member, size_t n, const char *what)
{
    const size_t bad = kws_pool_member_check(member, n, p->m.size());
    if (bad < n) return fail(KWS_ERROR_BAD_ARGUMENT, "%s %zu: member %u is at or above the pool's %zu", what, bad, member[bad], p->m.size());
    return EI_IMPULSE_OK;
}

// Items and lists travel with the call (one upload, behind the stream's earlier work: a chunk's table replaces the previous chunk's only
// after its launch); a member nobody names gets no item, and rows that all name KWS_POOL_NONE launch nothing.
EI_IMPULSE_ERROR pool_networks(kws_pool *p, const float *feat, size_t n, const uint32_t *member, float *scores, size_t row0, hipStream_t s)
{
    if (!scores || n == 0) return EI_IMPULSE_OK;
    EI_IMPULSE_ERROR e;
    if ((e = p->table.wait())) return e;
    const size_t n_items = kws_pool_items(member, n, p->m.size(), pool_item_rows(), p->table.host, p->fill);
    if (n_items == 0) return EI_IMPULSE_OK;
    const size_t total = p->table.host.size();
    if ((e = p->table.grow(total)) || (e = p->table.send(total, s))) return e;
    KWS_LAUNCH_TRY_OBJ("pool NN kernel", kws_launch_pool_nn_mfma(p->d_rec, (const KwsPoolItem *)p->table.dev, (int)n_items, p->table.dev + 4 * n_items, p->cp, feat,
                                                                scores + row0 * p->stride, (int)p->stride, s));
    return EI_IMPULSE_OK;
}

// where n feature rows of a call go: the caller's buffer, or (features == NULL) the pool's shared matrix, grown to hold them
static EI_IMPULSE_ERROR pool_feature_rows(kws_pool *p, float *features, size_t n, float **f)
{
    *f = features;
    if (features) return EI_IMPULSE_OK;
    const EI_IMPULSE_ERROR e = grow_buffer(&p->feat, &p->feat_cap, n * (size_t)p->m[0]->model.nn_input_frame_size);
    *f = p->feat;
    return e;
}

// The pool's lock and the first member's, and (bracket) that member's scratch bracket where no pipeline runner brackets it itself: the call
// is a call on those two and on no other member.
struct PoolUse {
    std::unique_lock<std::mutex> own, first;
    std::unique_ptr<ScratchUse> use;                       // released before the locks (declared after them)
    kws_pool *p;
    hipStream_t s;
    // held: the pool's own lock, already taken by the caller (a push that reads the session's members under it)
    PoolUse(kws_pool *p_, hipStream_t s_, bool bracket, std::unique_lock<std::mutex> &&held = std::unique_lock<std::mutex>()) : own(std::move(held)), p(p_), s(s_)
    {
        if (!own.owns_lock()) own = std::unique_lock<std::mutex>(p->mu);
        first = std::unique_lock<std::mutex>(p->m[0]->mu);
        if (bracket) use.reset(new ScratchUse(p->m[0], s));
    }
    ~PoolUse()
    {
        if (p->ev && hipEventRecord(p->ev, s) == hipSuccess) p->ev_used = true;
    }
};

// the end of the pool's latest call, a session's last push included (PoolUse records it), before memory it may read goes or changes
static void pool_wait(kws_pool *p)
{
    (void)hipSetDevice(p->device);
    if (p->ev && p->ev_used) (void)hipEventSynchronize(p->ev);
}

// What the finishing step of a call's rows needs: the rows' members (host), or the members of the call's entries -- a live push: the
// session's members by stream; a recording call: the call's members by recording (streams == NULL) -- from which the per-window table is
// built at the first non-empty chunk: every entry's window count is on the host before a hook is called (a push: the runner has filled
// the caller's n_windows; a recording call: counted before the runner starts), so nothing of the networks is enqueued before it, and each
// chunk is handed its part.
struct PoolWindows {
    kws_pool *p;
    float *scores;                         // [rows][stride] (NULL: no network)
    float *features;                       // the caller's [rows][F], or NULL: the pool's shared matrix, a chunk at a time
    const uint32_t *member = nullptr;      // [rows] (host)
    const uint32_t *assign = nullptr;      // the entries' members: a live push's session [S], a recording call's [R] ...
    const size_t *streams = nullptr, *n_windows = nullptr;     // ... and the entries' streams (NULL: entry i is recording i) and window counts
    size_t n = 0;
    std::vector<uint32_t> table;
    void by_entry(const uint32_t *assign_, const size_t *streams_, const size_t *n_windows_, size_t n_) { assign = assign_; streams = streams_; n_windows = n_windows_; n = n_; }
};

// the finishing step of a chunk of gathered windows: cmvnw (the MFE normalisation) once through the first member, then the windows' members
static EI_IMPULSE_ERROR pool_window_finish(void *ctx, float *win, size_t n, size_t g0, hipStream_t s)
{
    if (n == 0) return EI_IMPULSE_OK;
    PoolWindows &c = *(PoolWindows *)ctx;
    if (c.assign && !c.member) {
        kws_pool_window_members(c.assign, c.streams, c.n_windows, c.n, c.table);
        c.member = c.table.data();
    }
    float *f;
    EI_IMPULSE_ERROR e = pool_feature_rows(c.p, c.features ? c.features + g0 * c.p->m[0]->model.nn_input_frame_size : nullptr, n, &f);
    if (e) return e;
    if ((e = cmvn_nn_device(c.p->m[0], win, n, f, nullptr, nullptr, nullptr, nullptr, nullptr, s))) return e;
    return pool_networks(c.p, f, n, c.member + g0, c.scores, g0, s);
}

// the ragged call's finishing step: the DSP route has written the full-stride feature rows; the rows' members read them
static EI_IMPULSE_ERROR pool_ragged_finish(void *ctx, float *f, size_t B, size_t, hipStream_t s)
{
    PoolWindows &c = *(PoolWindows *)ctx;
    return pool_networks(c.p, f, B, c.member, c.scores, 0, s);
}

// Continuous mode: the chunks' raw scores go where the moving average reads them -- raw_scores, or scores (filtered in place) -- and the
// filter step is one launch over (entry, column) pairs.
struct PoolContinuous {
    PoolWindows w;                         // (first: pool_window_finish reads it)
    float *scores;
    int k_full;
    float *maf;
    const uint32_t *d_assign;
};
static EI_IMPULSE_ERROR pool_continuous_maf(void *ctx, const long long *meta, int n, hipStream_t s)
{
    PoolContinuous &c = *(PoolContinuous *)ctx;
    kws_pool *p = c.w.p;
    KWS_LAUNCH_TRY("pool moving-average kernel", kws_launch_pool_maf_live(c.w.scores, c.scores, meta, n, (int)p->stride, c.d_assign, p->d_labels, c.k_full, c.maf, s));
    return EI_IMPULSE_OK;
}

// A recording call's members: every recording's window count and, of the recordings that have windows, their members in order (what
// the scan's moving average reads, in the order of the runner's wbase); named: one of those is not KWS_POOL_NONE.
struct PoolRecordings {
    std::vector<size_t> n_windows;         // [R]
    std::vector<uint32_t> active;
    bool named = false;
    void add(uint32_t member, size_t W)
    {
        n_windows.push_back(W);
        if (!W) return;
        active.push_back(member);
        named = named || member != KWS_POOL_NONE;
    }
};

// The scan: raw scores as in a live push; the filter step is one launch over (recording with windows, column) pairs, a fresh filter each.
// The members travel with the call, behind the stream's earlier work, in an upload of their own (the table's host copy is the last chunk's).
struct PoolScan {
    PoolWindows w;                         // (first: pool_window_finish reads it)
    float *scores;
    const PoolRecordings *rec;
};
static EI_IMPULSE_ERROR pool_scan_maf(void *ctx, const long long *wbase, int n, hipStream_t s)
{
    PoolScan &c = *(PoolScan *)ctx;
    kws_pool *p = c.w.p;
    if (!c.rec->named) return EI_IMPULSE_OK;
    if ((size_t)n != c.rec->active.size()) return fail(KWS_ERROR_BAD_ARGUMENT, "pool scan: %d recordings with windows, %zu members", n, c.rec->active.size());
    EI_IMPULSE_ERROR e = p->scan_members.wait();
    if (e) return e;
    p->scan_members.host = c.rec->active;
    if ((e = p->scan_members.grow((size_t)n)) || (e = p->scan_members.send((size_t)n, s))) return e;
    KWS_LAUNCH_TRY("pool scan moving-average kernel", kws_launch_pool_maf_scan(c.w.scores, c.scores, wbase, n, (int)p->stride, p->scan_members.dev, p->d_labels, s));
    return EI_IMPULSE_OK;
}

// (the sessions: the pool, the first member's session -- carry, retained rows, mirrors, per-push scratch: ONE copy -- and the streams' members)
struct kws_pool_slide_live {
    kws_pool *p = nullptr;
    kws_slide_live *core = nullptr;
    std::vector<uint32_t> assign;          // [S]: the stream's member, or KWS_POOL_NONE (host only: nothing per member is kept)
};
struct kws_pool_live {
    kws_pool *p = nullptr;
    kws_live *core = nullptr;
    ScanLayout L;
    float *maf = nullptr;                  // state in HBM: [S][stride][taps + 1]
    std::vector<uint32_t> assign;          // [S]: the stream's member, or KWS_POOL_NONE
    uint32_t *d_assign = nullptr;          // the same in HBM, where the moving average reads it
    std::vector<char> pushed;              // [S]: the stream has been pushed to since its start (create, reset or finish): its member is fixed
};

static EI_IMPULSE_ERROR pool_call_checks(const kws_pool *p, const void *pcm, size_t B, const uint32_t *member, const float *scores, const float *features, bool need_pcm,
                                         const char *what = "clip")
{
    if (!p) return fail(KWS_ERROR_BAD_ARGUMENT, "null argument");
    if (!scores && !features) return fail(KWS_ERROR_BAD_ARGUMENT, "no output requested: scores and features are NULL");
    if (B >= ((size_t)1 << 31)) return fail(KWS_ERROR_BAD_ARGUMENT, "batch too large");
    if (B > 0 && (!member || (need_pcm && !pcm))) return fail(KWS_ERROR_BAD_ARGUMENT, "null argument");
    return pool_members_check(p, member, B, what);
}

extern "C" {
#pragma GCC visibility push(default)

EI_IMPULSE_ERROR kws_pool_create(kws_handle *const *members, size_t K, kws_pool **out)
{
    if (out) *out = nullptr;
    if (!members || !out) return fail(KWS_ERROR_BAD_ARGUMENT, "null argument");
    if (K < 1 || K > KWS_POOL_MAX) return fail(KWS_ERROR_BAD_ARGUMENT, "a pool has 1 to %d members, not %zu", KWS_POOL_MAX, K);
    {
        std::vector<kws_handle *> sorted(members, members + K);
        for (size_t k = 0; k < K; ++k)
            if (!members[k]) return fail(KWS_ERROR_BAD_ARGUMENT, "pool member %zu is NULL", k);
        // (distinct handles: sorted by address, then the first pair in the caller's order is named)
        std::sort(sorted.begin(), sorted.end(), std::less<kws_handle *>());
        if (std::adjacent_find(sorted.begin(), sorted.end()) != sorted.end())
            for (size_t k = 0; k < K; ++k)
                for (size_t j = 0; j < k; ++j)
                    if (members[j] == members[k]) return fail(KWS_ERROR_BAD_ARGUMENT, "pool members %zu and %zu are the same handle", j, k);
    }
    for (size_t k = 1; k < K; ++k) {
        EI_IMPULSE_ERROR e = bank_same_front_end(members[0], members[k], k);
        if (e) return e;
    }
    for (size_t k = 0; k < K; ++k) {
        const kws_handle *h = members[k];
        if (h->is_float) return fail(KWS_ERROR_UNSUPPORTED_MODEL, "pool member %zu is a float32 graph: a pool holds int8 graphs of the two-block matrix-core shape", k);
        if (!kws_pool_nn_fits(h->nn))
            return fail(KWS_ERROR_UNSUPPORTED_MODEL, "pool member %zu is an int8 graph outside the two-block matrix-core shape (%s serves it)", k, kws_nn_kernel_name(h));
        // (every member reads the same feature columns, so the plans agree on the activation-row width; one launch serves one width)
        if ((h->nn.blk[0].in_cpad == 16) != (members[0]->nn.blk[0].in_cpad == 16) || h->nn.n_features != members[0]->nn.n_features)
            return fail(KWS_ERROR_UNSUPPORTED_MODEL, "pool member %zu has activation rows of %d bytes, member 0 of %d", k, h->nn.blk[0].in_cpad, members[0]->nn.blk[0].in_cpad);
    }
    std::unique_ptr<kws_pool> p(new kws_pool());
    p->m.assign(members, members + K);
    p->device = members[0]->device;
    p->cp = members[0]->nn.blk[0].in_cpad == 16 ? 16 : 64;          // (kws_launch_nn's rule)
    HIP_TRY(hipSetDevice(p->device));
    std::vector<KwsBankRec> rec(K);
    std::vector<int> labels(K);
    for (size_t k = 0; k < K; ++k) {
        memset(&rec[k], 0, sizeof(KwsBankRec));
        rec[k].N = members[k]->nn;
        rec[k].in_scale = members[k]->nn.in_scale;
        rec[k].in_zp = members[k]->nn.in_zp;
        labels[k] = (int)members[k]->model.labels.size();
        if (members[k]->model.labels.size() > p->stride) {
            p->stride = members[k]->model.labels.size();
            p->most = k;
        }
    }
    hipError_t he = hipMalloc((void **)&p->d_rec, K * sizeof(KwsBankRec));
    if (he == hipSuccess) he = hipMalloc((void **)&p->d_labels, K * sizeof(int));
    if (he == hipSuccess) he = hipMemcpy(p->d_rec, rec.data(), K * sizeof(KwsBankRec), hipMemcpyHostToDevice);
    if (he == hipSuccess) he = hipMemcpy(p->d_labels, labels.data(), K * sizeof(int), hipMemcpyHostToDevice);
    if (he == hipSuccess) he = hipEventCreateWithFlags(&p->ev, hipEventDisableTiming);
    if (he != hipSuccess) {
        if (p->d_rec) (void)hipFree(p->d_rec);
        if (p->d_labels) (void)hipFree(p->d_labels);
        return fail(KWS_ERROR_HIP, "kws_pool_create: %s", hipGetErrorString(he));
    }
    *out = p.release();
    return EI_IMPULSE_OK;
}

void kws_pool_destroy(kws_pool *p)
{
    if (!p) return;
    (void)hipSetDevice(p->device);
    if (p->ev) {
        if (p->ev_used) (void)hipEventSynchronize(p->ev);
        (void)hipEventDestroy(p->ev);
    }
    if (p->d_rec) (void)hipFree(p->d_rec);
    if (p->d_labels) (void)hipFree(p->d_labels);
    if (p->feat) (void)hipFree(p->feat);
    p->table.release();
    p->scan_members.release();
    delete p;
}

size_t kws_pool_size(const kws_pool *p) { return p ? p->m.size() : 0; }
kws_handle *kws_pool_member(const kws_pool *p, size_t k) { return p && k < p->m.size() ? p->m[k] : nullptr; }
size_t kws_pool_score_stride(const kws_pool *p) { return p ? p->stride : 0; }
int kws_pool_item_rows(void) { return pool_item_rows(); }

EI_IMPULSE_ERROR kws_pool_run_classifier_device(kws_pool *p, const int16_t *pcm, size_t B, const uint32_t *member, float *scores, float *features, void *stream)
{
    EI_IMPULSE_ERROR e = pool_call_checks(p, pcm, B, member, scores, features, true);
    if (e) return e;
    if (B == 0) return EI_IMPULSE_OK;
    HIP_TRY(hipSetDevice(p->device));
    hipStream_t s = (hipStream_t)stream;
    PoolUse use(p, s, true);
    float *f;
    if ((e = pool_feature_rows(p, features, B, &f))) return e;
    if ((e = mfcc_fused_device(p->m[0], pcm, 0, B, f, nullptr, s))) return e;
    return pool_networks(p, f, B, member, scores, 0, s);
}

EI_IMPULSE_ERROR kws_pool_run_classifier_ragged_device(kws_pool *p, const int16_t *pcm, const size_t *offsets, const size_t *lengths, size_t B,
                                                       const uint32_t *member, float *scores, float *features, void *stream)
{
    // (pcm, offsets and lengths: the pipeline refuses what the single-model call refuses)
    EI_IMPULSE_ERROR e = pool_call_checks(p, pcm, B, member, scores, features, false);
    if (e) return e;
    if (B == 0) return EI_IMPULSE_OK;
    HIP_TRY(hipSetDevice(p->device));
    hipStream_t s = (hipStream_t)stream;
    PoolUse use(p, s, false);
    float *f;
    if ((e = pool_feature_rows(p, features, B, &f))) return e;
    PoolWindows ctx{ p, scores, features, member };
    return kws_ragged_run(p->m[0], pcm, offsets, lengths, B, f, nullptr, 0, 0, pool_ragged_finish, &ctx, s);
}

EI_IMPULSE_ERROR kws_pool_live_create(kws_pool *p, size_t S, size_t slice_samples, kws_pool_live **out)
{
    if (out) *out = nullptr;
    if (!p || !out) return fail(KWS_ERROR_BAD_ARGUMENT, "bad argument");
    std::unique_ptr<kws_pool_live> lv(new kws_pool_live());
    lv->p = p;
    EI_IMPULSE_ERROR e = kws_live_open(p->m[0], S, slice_samples, 0, &lv->core);
    if (e) return e;
    (void)scan_layout(p->m[0], slice_samples, &lv->L);             // (kws_live_open has accepted the slicing)
    lv->assign.assign(S, KWS_POOL_NONE);
    lv->pushed.assign(S, 0);
    const size_t maf_b = S * p->stride * (kPoolTaps + 1) * sizeof(float);
    // (a stream's filters are read only once it has had a window; cleared so that no stale value can ever reach a result)
    const bool ok = hipMalloc((void **)&lv->maf, maf_b) == hipSuccess && hipMemset(lv->maf, 0, maf_b) == hipSuccess &&
                    hipMalloc((void **)&lv->d_assign, S * sizeof(uint32_t)) == hipSuccess &&
                    hipMemcpy(lv->d_assign, lv->assign.data(), S * sizeof(uint32_t), hipMemcpyHostToDevice) == hipSuccess;
    if (!ok) {
        if (lv->maf) (void)hipFree(lv->maf);
        if (lv->d_assign) (void)hipFree(lv->d_assign);
        kws_live_destroy(lv->core);
        return fail(KWS_ERROR_HIP, "pool live session allocation failed");
    }
    *out = lv.release();
    return EI_IMPULSE_OK;
}

void kws_pool_live_destroy(kws_pool_live *lv)
{
    if (!lv) return;
    {
        std::lock_guard<std::mutex> lk(lv->p->mu);
        pool_wait(lv->p);
        kws_live_destroy(lv->core);
        if (lv->maf) (void)hipFree(lv->maf);
        if (lv->d_assign) (void)hipFree(lv->d_assign);
    }
    delete lv;
}

EI_IMPULSE_ERROR kws_pool_live_reset(kws_pool_live *lv, const size_t *streams, size_t n)
{
    if (!lv) return fail(KWS_ERROR_BAD_ARGUMENT, "null argument");
    std::lock_guard<std::mutex> lk(lv->p->mu);
    const EI_IMPULSE_ERROR e = kws_live_reset(lv->core, streams, n);
    if (e) return e;
    // (members stay; the streams are in their start state again, where a member may change)
    if (!streams) std::fill(lv->pushed.begin(), lv->pushed.end(), 0);
    else for (size_t i = 0; i < n; ++i) lv->pushed[streams[i]] = 0;
    return EI_IMPULSE_OK;
}

EI_IMPULSE_ERROR kws_pool_live_assign(kws_pool_live *lv, const size_t *streams, size_t n, const uint32_t *member)
{
    if (!lv) return fail(KWS_ERROR_BAD_ARGUMENT, "null argument");
    kws_pool *p = lv->p;
    std::lock_guard<std::mutex> lk(p->mu);
    if (n > 0 && (!streams || !member)) return fail(KWS_ERROR_BAD_ARGUMENT, "null argument");
    const size_t S = lv->assign.size(), K = p->m.size();
    std::vector<char> named(S, 0);
    for (size_t i = 0; i < n; ++i) {
        if (streams[i] >= S) return fail(KWS_ERROR_BAD_ARGUMENT, "entry %zu: stream %zu of %zu", i, streams[i], S);
        if (named[streams[i]]) return fail(KWS_ERROR_BAD_ARGUMENT, "entry %zu: stream %zu named twice", i, streams[i]);
        named[streams[i]] = 1;
        if (member[i] >= K && member[i] != KWS_POOL_NONE) return fail(KWS_ERROR_BAD_ARGUMENT, "entry %zu: member %u is at or above the pool's %zu", i, member[i], K);
    }
    // the moving-average filter of a stream must see every window of it through one member: no change once the stream has been pushed to
    for (size_t i = 0; i < n; ++i)
        if (lv->pushed[streams[i]])
            return fail(KWS_ERROR_BAD_ARGUMENT, "entry %zu: stream %zu has been pushed to; its member changes only after a reset", i, streams[i]);
    if (n == 0) return EI_IMPULSE_OK;
    // (a push enqueued earlier may still read the old table: the pool's event marks the end of its latest call)
    pool_wait(p);
    std::vector<uint32_t> next = lv->assign;
    for (size_t i = 0; i < n; ++i) next[streams[i]] = member[i];
    HIP_TRY(hipMemcpy(lv->d_assign, next.data(), S * sizeof(uint32_t), hipMemcpyHostToDevice));
    lv->assign.swap(next);
    return EI_IMPULSE_OK;
}

EI_IMPULSE_ERROR kws_pool_live_window_count(const kws_pool_live *lv, size_t stream, size_t n_new, int finish, size_t *n_windows)
{
    if (!lv) return fail(KWS_ERROR_BAD_ARGUMENT, "null argument");
    std::lock_guard<std::mutex> lk(lv->p->mu);
    return kws_live_window_count(lv->core, stream, n_new, finish, n_windows);
}

EI_IMPULSE_ERROR kws_pool_live_push_device(kws_pool_live *lv, size_t n, const size_t *streams, const int16_t *pcm, const size_t *offsets, const size_t *lengths,
                                           const int *finish, float *scores, float *raw_scores, size_t *n_windows, void *stream)
{
    if (!lv) return fail(KWS_ERROR_BAD_ARGUMENT, "null argument");
    kws_pool *p = lv->p;
    std::unique_lock<std::mutex> own(p->mu);
    HIP_TRY(hipSetDevice(p->device));
    hipStream_t s = (hipStream_t)stream;
    PoolUse use(p, s, false, std::move(own));
    PoolContinuous ctx{ { p, raw_scores ? raw_scores : scores, nullptr }, scores, (int)lv->L.k_full, lv->maf, lv->d_assign };
    ctx.w.by_entry(lv->assign.data(), streams, n_windows, n);
    const EI_IMPULSE_ERROR e = kws_live_run(lv->core, n, streams, pcm, offsets, lengths, finish, scores, n_windows, p->stride, 0, 0, pool_window_finish,
                                            pool_continuous_maf, &ctx, s);
    if (e) return e;
    // (a stream the push finished starts over: its member may change again)
    for (size_t i = 0; i < n; ++i) lv->pushed[streams[i]] = !(finish && finish[i]);
    return EI_IMPULSE_OK;
}

EI_IMPULSE_ERROR kws_pool_cmvn_inference_device(kws_pool *p, const float *mfcc, size_t B, const uint32_t *member, float *scores, float *features, void *stream)
{
    EI_IMPULSE_ERROR e = pool_call_checks(p, mfcc, B, member, scores, features, true, "row");
    if (e) return e;
    if (B == 0) return EI_IMPULSE_OK;
    HIP_TRY(hipSetDevice(p->device));
    hipStream_t s = (hipStream_t)stream;
    PoolUse use(p, s, true);
    float *f;
    if ((e = pool_feature_rows(p, features, B, &f))) return e;
    if ((e = ensure_scratch(p->m[0], B))) return e;
    if ((e = cmvn_nn_device(p->m[0], mfcc, B, f, nullptr, nullptr, nullptr, nullptr, nullptr, s))) return e;
    return pool_networks(p, f, B, member, scores, 0, s);
}

EI_IMPULSE_ERROR kws_pool_scan_recordings_device(kws_pool *p, const int16_t *pcm, const size_t *offsets, const size_t *lengths, size_t R, const uint32_t *member,
                                                 size_t slice_samples, float *scores, float *raw_scores, void *stream)
{
    if (!p || !scores) return fail(KWS_ERROR_BAD_ARGUMENT, "null argument");
    // (the members are sorted out before the pipeline runs, so what it would refuse of the arguments read here is refused here)
    if (R > 0 && (!pcm || !offsets || !lengths || !member)) return fail(KWS_ERROR_BAD_ARGUMENT, "null argument");
    if (R > 0x3fffffff) return fail(KWS_ERROR_BAD_ARGUMENT, "too many recordings");
    EI_IMPULSE_ERROR e = pool_members_check(p, member, R, "recording");
    if (e) return e;
    ScanLayout L;
    if ((e = scan_layout(p->m[0], slice_samples, &L))) return e;
    PoolRecordings rec;
    for (size_t r = 0; r < R; ++r) rec.add(member[r], L.windows(lengths[r] / slice_samples));
    HIP_TRY(hipSetDevice(p->device));
    hipStream_t s = (hipStream_t)stream;
    PoolUse use(p, s, false);
    PoolScan ctx{ { p, raw_scores ? raw_scores : scores, nullptr }, scores, &rec };
    ctx.w.by_entry(member, nullptr, rec.n_windows.data(), R);
    return kws_scan_run(p->m[0], pcm, offsets, lengths, R, slice_samples, p->stride, 0, pool_window_finish, pool_scan_maf, &ctx, s);
}

EI_IMPULSE_ERROR kws_pool_slide_recordings_device(kws_pool *p, const int16_t *pcm, const size_t *offsets, const size_t *lengths, size_t R, const uint32_t *member,
                                                  size_t hop_samples, int flags, float *scores, float *features, void *stream)
{
    if (!p) return fail(KWS_ERROR_BAD_ARGUMENT, "null argument");
    if (!scores && !features) return fail(KWS_ERROR_BAD_ARGUMENT, "no output requested: scores and features are NULL");
    // the window count is any member's; the bound on windows x labels holds at the stride, the label count of member `most` (a bad hop or
    // flags, NULL lengths, too many windows: its plan refuses them)
    kws_slide_plan_info I;
    EI_IMPULSE_ERROR e = kws_slide_plan(p->m[p->most], lengths, R, hop_samples, flags, &I);
    if (e) return e;
    if (R > 0 && (!pcm || !offsets || !member)) return fail(KWS_ERROR_BAD_ARGUMENT, "null argument");
    if ((e = pool_members_check(p, member, R, "recording"))) return e;
    PoolRecordings rec;
    for (size_t r = 0; r < R; ++r) {
        size_t W = 0;
        if ((e = kws_slide_window_count(p->m[0], lengths[r], hop_samples, &W))) return e;
        rec.add(member[r], W);
    }
    HIP_TRY(hipSetDevice(p->device));
    hipStream_t s = (hipStream_t)stream;
    PoolUse use(p, s, false);
    PoolWindows ctx{ p, scores, features };
    ctx.by_entry(member, nullptr, rec.n_windows.data(), R);
    return kws_slide_run(p->m[0], pcm, offsets, lengths, R, hop_samples, flags, 0, pool_window_finish, &ctx, s);
}

EI_IMPULSE_ERROR kws_pool_slide_live_create(kws_pool *p, size_t S, size_t hop_samples, int flags, kws_pool_slide_live **out)
{
    if (out) *out = nullptr;
    if (!p || !out) return fail(KWS_ERROR_BAD_ARGUMENT, "bad argument");
    std::unique_ptr<kws_pool_slide_live> sl(new kws_pool_slide_live());
    sl->p = p;
    EI_IMPULSE_ERROR e = kws_slide_live_create(p->m[0], S, hop_samples, flags, &sl->core);
    if (e) return e;
    sl->assign.assign(S, KWS_POOL_NONE);
    *out = sl.release();
    return EI_IMPULSE_OK;
}

void kws_pool_slide_live_destroy(kws_pool_slide_live *sl)
{
    if (!sl) return;
    {
        std::lock_guard<std::mutex> lk(sl->p->mu);
        pool_wait(sl->p);
        kws_slide_live_destroy(sl->core);
    }
    delete sl;
}

int kws_pool_slide_live_path(const kws_pool_slide_live *sl) { return sl ? kws_slide_live_path(sl->core) : 0; }

EI_IMPULSE_ERROR kws_pool_slide_live_reset(kws_pool_slide_live *sl, const size_t *streams, size_t n)
{
    if (!sl) return fail(KWS_ERROR_BAD_ARGUMENT, "null argument");
    std::lock_guard<std::mutex> lk(sl->p->mu);
    return kws_slide_live_reset(sl->core, streams, n);          // (members stay)
}

EI_IMPULSE_ERROR kws_pool_slide_live_assign(kws_pool_slide_live *sl, const size_t *streams, size_t n, const uint32_t *member)
{
    if (!sl) return fail(KWS_ERROR_BAD_ARGUMENT, "null argument");
    std::lock_guard<std::mutex> lk(sl->p->mu);
    if (n > 0 && (!streams || !member)) return fail(KWS_ERROR_BAD_ARGUMENT, "null argument");
    const size_t S = sl->assign.size(), K = sl->p->m.size();
    std::vector<char> named(S, 0);
    for (size_t i = 0; i < n; ++i) {
        if (streams[i] >= S) return fail(KWS_ERROR_BAD_ARGUMENT, "entry %zu: stream %zu of %zu", i, streams[i], S);
        if (named[streams[i]]) return fail(KWS_ERROR_BAD_ARGUMENT, "entry %zu: stream %zu named twice", i, streams[i]);
        named[streams[i]] = 1;
        if (member[i] >= K && member[i] != KWS_POOL_NONE) return fail(KWS_ERROR_BAD_ARGUMENT, "entry %zu: member %u is at or above the pool's %zu", i, member[i], K);
    }
    // (no per-member state and no device table: a push reads the members on the host, under the pool's lock, so a member may change
    // between any two pushes)
    for (size_t i = 0; i < n; ++i) sl->assign[streams[i]] = member[i];
    return EI_IMPULSE_OK;
}

EI_IMPULSE_ERROR kws_pool_slide_live_window_count(const kws_pool_slide_live *sl, size_t stream, size_t n_new, size_t *n_windows)
{
    if (!sl) return fail(KWS_ERROR_BAD_ARGUMENT, "null argument");
    std::lock_guard<std::mutex> lk(sl->p->mu);
    return kws_slide_live_window_count(sl->core, stream, n_new, n_windows);
}

EI_IMPULSE_ERROR kws_pool_slide_live_push_device(kws_pool_slide_live *sl, size_t n, const size_t *streams, const int16_t *pcm, const size_t *offsets,
                                                 const size_t *lengths, float *scores, float *features, size_t *n_windows, void *stream)
{
    if (!sl) return fail(KWS_ERROR_BAD_ARGUMENT, "null argument");
    if (!scores && !features) return fail(KWS_ERROR_BAD_ARGUMENT, "no output requested: scores and features are NULL");
    kws_pool *p = sl->p;
    std::unique_lock<std::mutex> own(p->mu);
    HIP_TRY(hipSetDevice(p->device));
    hipStream_t s = (hipStream_t)stream;
    PoolUse use(p, s, false, std::move(own));
    PoolWindows ctx{ p, scores, features };
    ctx.by_entry(sl->assign.data(), streams, n_windows, n);
    return kws_slide_live_run(sl->core, n, streams, pcm, offsets, lengths, scores ? scores : features, n_windows, p->stride, 0, 0, pool_window_finish, &ctx, s);
}

#pragma GCC visibility pop
}
