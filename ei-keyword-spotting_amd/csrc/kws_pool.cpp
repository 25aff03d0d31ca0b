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

void kws_pool_window_members(const uint32_t *assign, const size_t *streams, const size_t *n_windows, size_t n, std::vector<uint32_t> &out)
{
    out.clear();
    for (size_t i = 0; i < n; ++i) out.insert(out.end(), n_windows[i], assign[streams[i]]);
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

// What the finishing step of a call's rows needs: the rows' members (host), or -- a live push -- the session's members by stream, from
// which the per-window table is built at the first non-empty chunk: every entry's window count is on the host before a hook is called (the
// runner has filled the caller's n_windows), so nothing of the networks is enqueued before it, and each chunk is handed its part.
struct PoolWindows {
    kws_pool *p;
    float *scores;                         // [rows][stride] (NULL: no network)
    float *features;                       // the caller's [rows][F], or NULL: the pool's shared matrix, a chunk at a time
    const uint32_t *member = nullptr;      // [rows] (host)
    const uint32_t *assign = nullptr;      // a live push: the session's members [S] ...
    const size_t *streams = nullptr, *n_windows = nullptr;     // ... and the entries' streams and window counts
    size_t n = 0;
    std::vector<uint32_t> table;
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

// (the session: the pool, the first member's session -- carry, retained rows, mirrors, per-push scratch: ONE copy -- and the streams' members)
struct kws_pool_live {
    kws_pool *p = nullptr;
    kws_live *core = nullptr;
    ScanLayout L;
    float *maf = nullptr;                  // state in HBM: [S][stride][taps + 1]
    std::vector<uint32_t> assign;          // [S]: the stream's member, or KWS_POOL_NONE
    uint32_t *d_assign = nullptr;          // the same in HBM, where the moving average reads it
    std::vector<char> pushed;              // [S]: the stream has been pushed to since its start (create, reset or finish): its member is fixed
};

static EI_IMPULSE_ERROR pool_call_checks(const kws_pool *p, const void *pcm, size_t B, const uint32_t *member, const float *scores, const float *features, bool need_pcm)
{
    if (!p) return fail(KWS_ERROR_BAD_ARGUMENT, "null argument");
    if (!scores && !features) return fail(KWS_ERROR_BAD_ARGUMENT, "no output requested: scores and features are NULL");
    if (B >= ((size_t)1 << 31)) return fail(KWS_ERROR_BAD_ARGUMENT, "batch too large");
    if (B > 0 && (!member || (need_pcm && !pcm))) return fail(KWS_ERROR_BAD_ARGUMENT, "null argument");
    return pool_members_check(p, member, B, "clip");
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
        p->stride = std::max(p->stride, members[k]->model.labels.size());
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
    ctx.w.assign = lv->assign.data();
    ctx.w.streams = streams;
    ctx.w.n_windows = n_windows;
    ctx.w.n = n;
    const EI_IMPULSE_ERROR e = kws_live_run(lv->core, n, streams, pcm, offsets, lengths, finish, scores, n_windows, p->stride, 0, 0, pool_window_finish,
                                            pool_continuous_maf, &ctx, s);
    if (e) return e;
    // (a stream the push finished starts over: its member may change again)
    for (size_t i = 0; i < n; ++i) lv->pushed[streams[i]] = !(finish && finish[i]);
    return EI_IMPULSE_OK;
}

#pragma GCC visibility pop
}
