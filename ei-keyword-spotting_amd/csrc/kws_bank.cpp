// kws_bank.cpp -- banks: K model handles with an identical DSP block scored in one call (kws_bank_*; contract in include/kws/kws.h).
//
// A bank call runs the DSP block ONCE, through the first member and with that member's own exact launches (mfcc_fused_device for clips;
// cmvn_nn_device without a network for cepstra and for the slide's gathered windows), into one float feature matrix, and every member's
// network from that matrix:
//   int8, two-block matrix-core shape (kws_nn_uses_mfma)  kws_bank_nn_mfma_kernel: one launch per activation-row width for all of them,
//                                                         quantising on load (kws_bank_kernels.hip)
//   other int8 graphs                                     kws_bank_quantize_kernel writes all their input tensors in one pass, into each
//                                                         member's scratch; then the member's own network_device
//   float32 graphs                                        the member's own network_device on the shared matrix, no logits tap
// Nothing here reads a member's mode, fast counters or tap: these are the launches of KWS_MODE_EXACT.
#include "kws_internal.h"
#include "kws_bank.h"

#include <algorithm>

#define DIFFER(field, fmt, a, b_)                                                                                                      \
    return fail(KWS_ERROR_BAD_ARGUMENT, "bank member %zu differs from member 0 in " field ": " fmt " against " fmt, k, a, b_)

// (also the membership rule of a pool: kws_pool.cpp)
EI_IMPULSE_ERROR bank_same_front_end(const kws_handle *a, const kws_handle *h, size_t k)
{
    const Model &x = a->model, &y = h->model;
    const DspCfg &p = x.dsp, &q = y.dsp;
    if (a->device != h->device) DIFFER("device", "%d", h->device, a->device);
    if (p.block != q.block) DIFFER("DSP block kind", "%d", q.block, p.block);
    if (p.axes != q.axes) DIFFER("axes", "%d", q.axes, p.axes);
    if (p.num_cepstral != q.num_cepstral) DIFFER("num_cepstral", "%d", q.num_cepstral, p.num_cepstral);
    if (p.frame_length != q.frame_length) DIFFER("frame_length", "%g", (double)q.frame_length, (double)p.frame_length);
    if (p.frame_stride != q.frame_stride) DIFFER("frame_stride", "%g", (double)q.frame_stride, (double)p.frame_stride);
    if (p.num_filters != q.num_filters) DIFFER("num_filters", "%d", q.num_filters, p.num_filters);
    if (p.fft_length != q.fft_length) DIFFER("fft_length", "%d", q.fft_length, p.fft_length);
    if (p.win_size != q.win_size) DIFFER("win_size", "%d", q.win_size, p.win_size);
    if (p.low_frequency != q.low_frequency) DIFFER("low_frequency", "%d", q.low_frequency, p.low_frequency);
    if (p.high_frequency != q.high_frequency) DIFFER("high_frequency", "%d", q.high_frequency, p.high_frequency);
    if (p.pre_cof != q.pre_cof) DIFFER("pre_cof", "%g", (double)q.pre_cof, (double)p.pre_cof);
    if (p.pre_shift != q.pre_shift) DIFFER("pre_shift", "%d", q.pre_shift, p.pre_shift);
    if (p.quantize_fb != q.quantize_fb) DIFFER("EIDSP_QUANTIZE_FILTERBANK", "%d", q.quantize_fb, p.quantize_fb);
    if (x.frequency != y.frequency) DIFFER("sampling frequency", "%u", y.frequency, x.frequency);
    if (x.raw_sample_count != y.raw_sample_count) DIFFER("raw_sample_count", "%u", y.raw_sample_count, x.raw_sample_count);
    // (what follows from the above; a blob that contradicts itself is refused here rather than trusted)
    if (x.nn_input_frame_size != y.nn_input_frame_size || a->dsp.n_frames != h->dsp.n_frames || a->dsp.n_cepstral != h->dsp.n_cepstral)
        DIFFER("feature matrix", "%u values", y.nn_input_frame_size, x.nn_input_frame_size);
    return EI_IMPULSE_OK;
}

// Routes to lists, as host arithmetic: one counting pass over the routes sizes the K lists, a second one fills them in row order, so every
// list is ascending.  Member k's list is out[at[k]] = its count, then its rows; at[K] = the packed size.
void kws_bank_route_lists(const uint32_t *routes, size_t n, size_t K, std::vector<int> &out, size_t *at)
{
    size_t count[KWS_BANK_MAX] = { 0 };
    for (size_t i = 0; i < n; ++i)
        for (uint32_t r = routes[i] & ((1u << K) - 1u); r; r &= r - 1) ++count[__builtin_ctz(r)];
    at[0] = 0;
    for (size_t k = 0; k < K; ++k) at[k + 1] = at[k] + 1 + count[k];
    out.resize(at[K]);
    size_t fill[KWS_BANK_MAX];
    for (size_t k = 0; k < K; ++k) { out[at[k]] = (int)count[k]; fill[k] = at[k] + 1; }
    for (size_t i = 0; i < n; ++i)
        for (uint32_t r = routes[i] & ((1u << K) - 1u); r; r &= r - 1) out[fill[__builtin_ctz(r)]++] = (int)i;
}

size_t kws_bank_route_check(const uint32_t *routes, size_t n, size_t K)
{
    for (size_t i = 0; i < n; ++i)
        if (routes[i] >> K) return i;
    return n;
}

// the refusal of a call whose routes (NULL: none to check) name a member the bank does not have; what: the call's word for a row
EI_IMPULSE_ERROR bank_routes_check(const kws_bank *b, const uint32_t *routes, size_t n, const char *what)
{
    const size_t bad = routes ? kws_bank_route_check(routes, n, b->m.size()) : n;
    if (bad < n) return fail(KWS_ERROR_BAD_ARGUMENT, "%s %zu: route 0x%x names a member at or above the bank's %zu", what, bad, routes[bad], b->m.size());
    return EI_IMPULSE_OK;
}

// a launch of bank_networks, with the failure text of its form (reads `routed`): "bank <what> launch failed: ..." / "routed bank <what> ..."
#define BANK_LAUNCH_TRY(TRY, what, expr)             \
    do {                                             \
        const int rc = (expr);                       \
        if (routed) TRY("routed bank " what, rc);    \
        else TRY("bank " what, rc);                  \
    } while (0)

// Every member's network from the feature matrix feat [B][F] (device); scores[k] + row0 * labels of member k is where its rows go.  The int8
// members fall into three classes, one launch each: matrix-core with 16-byte activation rows, matrix-core with up to 64 (kws_launch_nn's
// rule), and the rest, whose input tensors one quantise pass writes before each runs its own network_device, as the float32 members do.
// Routed (some route does not name every member), member k runs over the list of rows that name it: the lists travel with the call (one
// upload, behind the stream's earlier work: a chunk's lists replace the previous chunk's only after its launches), and a member with an
// empty list, or without a score buffer, launches nothing.
EI_IMPULSE_ERROR bank_networks(kws_bank *b, const float *feat, size_t B, float *const *scores, size_t row0, hipStream_t s, const uint32_t *routes)
{
    const size_t K = b->m.size(), F = b->m[0]->model.nn_input_frame_size;
    // (routes that all name every member: the unrouted launches, which need no list)
    bool routed = false;
    for (size_t i = 0; routes && i < B; ++i) routed = routed || routes[i] != (1u << K) - 1u;
    size_t at[KWS_BANK_MAX + 1] = { 0 };
    EI_IMPULSE_ERROR e;
    if (routed) {
        if ((e = b->lists.wait())) return e;
        kws_bank_route_lists(routes, B, K, b->lists.host, at);
        if ((e = b->lists.grow(at[K]))) return e;
    }
    // member k's rows: how many, and which (NULL: all B)
    auto rows = [&](size_t k) { return !scores[k] ? 0 : routed ? b->lists.host[at[k]] : (int)B; };
    auto list = [&](size_t k) { return routed ? b->lists.dev + at[k] : (const int *)nullptr; };
    enum { W16, W64, QUANT, CLASSES };
    KwsBankOut o[2] = {};
    KwsBankQuant Q{};
    KwsBankLists l[CLASSES] = {};
    int longest[CLASSES] = { 0 }, own[KWS_BANK_MAX], n_own = 0;
    bool any = false;
    for (size_t k = 0; k < K; ++k) {
        kws_handle *h = b->m[k];
        if (rows(k) == 0) continue;
        any = true;
        const int c = h->is_float ? CLASSES : !kws_nn_uses_mfma(h->nn) ? QUANT : h->nn.blk[0].in_cpad == 16 ? W16 : W64;
        if (c >= QUANT) own[n_own++] = (int)k;
        if (c == CLASSES) continue;
        if (c == QUANT) {
            if ((e = ensure_scratch(h, B))) return e;         // (its tensor is indexed by row: B rows, routed the listed ones written)
            l[c].list[Q.n] = list(k);
            Q.scale[Q.n] = h->nn.in_scale; Q.zp[Q.n] = h->nn.in_zp; Q.q[Q.n] = h->s_q; ++Q.n;
        } else {
            l[c].list[o[c].n] = list(k);
            o[c].rec[o[c].n] = (int)k; o[c].scores[o[c].n] = scores[k] + row0 * h->model.labels.size(); ++o[c].n;
        }
        longest[c] = std::max(longest[c], rows(k));
    }
    if (!any) return EI_IMPULSE_OK;
    if (routed && (e = b->lists.send(at[K], s))) return e;
    const int grid_cap = grid_cap_nn(b->m[0]);
    BANK_LAUNCH_TRY(KWS_LAUNCH_TRY_OBJ, "NN kernel", kws_launch_bank_nn_mfma(b->d_rec, o[W16], routed ? &l[W16] : nullptr, 16, feat, longest[W16], grid_cap, s));
    BANK_LAUNCH_TRY(KWS_LAUNCH_TRY_OBJ, "NN kernel", kws_launch_bank_nn_mfma(b->d_rec, o[W64], routed ? &l[W64] : nullptr, 64, feat, longest[W64], grid_cap, s));
    BANK_LAUNCH_TRY(KWS_LAUNCH_TRY, "quantise kernel", kws_launch_bank_quantize(feat, longest[QUANT], (int)F, Q, routed ? &l[QUANT] : nullptr, s));
    for (int j = 0; j < n_own; ++j) {
        kws_handle *h = b->m[own[j]];
        float *dst = scores[own[j]] + row0 * h->model.labels.size();
        if ((e = network_device(h, feat, h->s_q, (size_t)rows(own[j]), dst, nullptr, nullptr, nullptr, nullptr, list(own[j]), s))) return e;
    }
    return EI_IMPULSE_OK;
}

bool bank_wants_nothing(const kws_bank *b, float *const *scores, const float *features)
{
    if (features) return false;
    for (size_t k = 0; k < b->m.size(); ++k) if (scores[k]) return false;
    return true;
}

EI_IMPULSE_ERROR bank_feature_rows(kws_bank *b, float *features, size_t n, float **f)
{
    *f = features;
    if (features) return EI_IMPULSE_OK;
    const EI_IMPULSE_ERROR e = grow_buffer(&b->feat, &b->feat_cap, n * (size_t)b->m[0]->model.nn_input_frame_size);
    *f = b->feat;
    return e;
}

// The two batch calls: the checks, the front end ONCE through the first member (front: from `in` into the feature matrix), then every
// member's network.  row: the call's word for a row in its refusals.
template <typename Front>
static EI_IMPULSE_ERROR bank_batch(kws_bank *b, const void *in, size_t B, const uint32_t *routes, const char *row, float *const *scores, float *features,
                                   void *stream, Front front)
{
    if (!b || !in || !scores) return fail(KWS_ERROR_BAD_ARGUMENT, "null argument");
    if (bank_wants_nothing(b, scores, features)) return fail(KWS_ERROR_BAD_ARGUMENT, "no output requested: every scores[k] and features are NULL");
    if (B > 0x7fffffff) return fail(KWS_ERROR_BAD_ARGUMENT, "batch too large");
    EI_IMPULSE_ERROR e = bank_routes_check(b, routes, B, row);
    if (e) return e;
    if (B == 0) return EI_IMPULSE_OK;
    HIP_TRY(hipSetDevice(b->device));
    hipStream_t s = (hipStream_t)stream;
    BankUse use(b, s, false);
    float *f;
    if ((e = bank_feature_rows(b, features, B, &f))) return e;
    if ((e = front(b->m[0], f, s))) return e;
    return bank_networks(b, f, B, scores, 0, s, routes);
}

extern "C" {
#pragma GCC visibility push(default)

EI_IMPULSE_ERROR kws_bank_create(kws_handle *const *members, size_t K, kws_bank **out)
{
    if (!members || !out) return fail(KWS_ERROR_BAD_ARGUMENT, "null argument");
    *out = nullptr;
    if (K < 1 || K > KWS_BANK_MAX) return fail(KWS_ERROR_BAD_ARGUMENT, "a bank has 1 to %d members, not %zu", KWS_BANK_MAX, K);
    for (size_t k = 0; k < K; ++k) {
        if (!members[k]) return fail(KWS_ERROR_BAD_ARGUMENT, "bank member %zu is NULL", k);
        for (size_t j = 0; j < k; ++j)
            if (members[j] == members[k]) return fail(KWS_ERROR_BAD_ARGUMENT, "bank members %zu and %zu are the same handle", j, k);
    }
    for (size_t k = 1; k < K; ++k) {
        EI_IMPULSE_ERROR e = bank_same_front_end(members[0], members[k], k);
        if (e) return e;
    }
    std::unique_ptr<kws_bank> b(new kws_bank());
    b->m.assign(members, members + K);
    b->by_addr = b->m;
    std::sort(b->by_addr.begin(), b->by_addr.end(), std::less<kws_handle *>());
    b->device = members[0]->device;
    HIP_TRY(hipSetDevice(b->device));
    std::vector<KwsBankRec> rec(K);
    for (size_t k = 0; k < K; ++k) {
        memset(&rec[k], 0, sizeof(KwsBankRec));
        if (members[k]->is_float) continue;
        rec[k].N = members[k]->nn;
        rec[k].in_scale = members[k]->nn.in_scale;
        rec[k].in_zp = members[k]->nn.in_zp;
    }
    HIP_TRY(hipMalloc((void **)&b->d_rec, K * sizeof(KwsBankRec)));
    hipError_t he = hipMemcpy(b->d_rec, rec.data(), K * sizeof(KwsBankRec), hipMemcpyHostToDevice);
    if (he == hipSuccess) he = hipEventCreateWithFlags(&b->ev, hipEventDisableTiming);
    if (he != hipSuccess) {
        (void)hipFree(b->d_rec);
        return fail(KWS_ERROR_HIP, "kws_bank_create: %s", hipGetErrorString(he));
    }
    *out = b.release();
    return EI_IMPULSE_OK;
}

void kws_bank_destroy(kws_bank *b)
{
    if (!b) return;
    (void)hipSetDevice(b->device);
    if (b->ev) {
        if (b->ev_used) (void)hipEventSynchronize(b->ev);
        (void)hipEventDestroy(b->ev);
    }
    if (b->d_rec) (void)hipFree(b->d_rec);
    if (b->feat) (void)hipFree(b->feat);
    b->lists.release();
    b->routes.release();
    delete b;
}

size_t kws_bank_size(const kws_bank *b) { return b ? b->m.size() : 0; }
kws_handle *kws_bank_member(const kws_bank *b, size_t k) { return b && k < b->m.size() ? b->m[k] : nullptr; }

EI_IMPULSE_ERROR kws_bank_run_classifier_batch_device(kws_bank *b, const int16_t *pcm, size_t B, float *const *scores, float *features, void *stream)
{
    return kws_bank_run_classifier_routed_device(b, pcm, B, nullptr, scores, features, stream);
}

EI_IMPULSE_ERROR kws_bank_run_classifier_routed_device(kws_bank *b, const int16_t *pcm, size_t B, const uint32_t *routes, float *const *scores, float *features,
                                                       void *stream)
{
    return bank_batch(b, pcm, B, routes, "clip", scores, features, stream,
                      [&](kws_handle *h0, float *f, hipStream_t s) { return mfcc_fused_device(h0, pcm, 0, B, f, nullptr, s); });
}

EI_IMPULSE_ERROR kws_bank_cmvn_inference_batch_device(kws_bank *b, const float *mfcc, size_t B, float *const *scores, float *features, void *stream)
{
    return kws_bank_cmvn_inference_routed_device(b, mfcc, B, nullptr, scores, features, stream);
}

EI_IMPULSE_ERROR kws_bank_cmvn_inference_routed_device(kws_bank *b, const float *mfcc, size_t B, const uint32_t *routes, float *const *scores, float *features, void *stream)
{
    return bank_batch(b, mfcc, B, routes, "row", scores, features, stream, [&](kws_handle *h0, float *f, hipStream_t s) {
        const EI_IMPULSE_ERROR e = ensure_scratch(h0, B);          // (a general-shape int8 first member: cmvn_nn_device writes its int8 tensor there)
        return e ? e : cmvn_nn_device(h0, mfcc, B, f, nullptr, nullptr, nullptr, nullptr, nullptr, s);
    });
}

#pragma GCC visibility pop
}
