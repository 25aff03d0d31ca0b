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

static EI_IMPULSE_ERROR bank_same_front_end(const kws_handle *a, const kws_handle *h, size_t k)
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

void kws_bank_window_routes(const uint32_t *route, const size_t *index, const size_t *n_windows, size_t n, std::vector<uint32_t> &out)
{
    out.clear();
    for (size_t i = 0; i < n; ++i) out.insert(out.end(), n_windows[i], route[index ? index[i] : i]);
}

// The routed form of bank_networks: member k runs over the rows whose route names it.  The lists travel with the call (one upload, behind
// the stream's earlier work: a chunk's lists replace the previous chunk's only after its launches); a member with an empty list, or without
// a score buffer, launches nothing.
static EI_IMPULSE_ERROR bank_networks_routed(kws_bank *b, const float *feat, size_t B, float *const *scores, size_t row0, const uint32_t *routes, hipStream_t s)
{
    const size_t K = b->m.size(), F = b->m[0]->model.nn_input_frame_size;
    size_t at[KWS_BANK_MAX + 1];
    // (the host copy is read by the upload of the call or chunk before: that upload has ended before it is rewritten)
    if (b->lists_ev_used) HIP_TRY(hipEventSynchronize(b->lists_ev));
    b->lists_ev_used = false;
    kws_bank_route_lists(routes, B, K, b->h_lists, at);
    EI_IMPULSE_ERROR e;
    if ((e = grow_buffer(&b->d_lists, &b->lists_cap, at[K]))) return e;
    KwsBankOut o16{}, o64{};
    KwsBankLists l16{}, l64{}, lq{};
    KwsBankQuant Q{};
    int n16 = 0, n64 = 0, nq = 0;
    bool any = false;
    for (size_t k = 0; k < K; ++k) {
        kws_handle *h = b->m[k];
        const int n = b->h_lists[at[k]];
        if (!scores[k] || n == 0) continue;
        any = true;
        if (h->is_float) continue;
        if (kws_nn_uses_mfma(h->nn)) {
            const bool w16 = h->nn.blk[0].in_cpad == 16;
            KwsBankOut &o = w16 ? o16 : o64;
            (w16 ? l16 : l64).list[o.n] = b->d_lists + at[k];
            (w16 ? n16 : n64) = std::max(w16 ? n16 : n64, n);
            o.rec[o.n] = (int)k; o.scores[o.n] = scores[k] + row0 * h->model.labels.size(); ++o.n;
        } else {
            if ((e = ensure_scratch(h, B))) return e;         // (its tensor is indexed by row: B rows, the listed ones written)
            lq.list[Q.n] = b->d_lists + at[k];
            nq = std::max(nq, n);
            Q.scale[Q.n] = h->nn.in_scale; Q.zp[Q.n] = h->nn.in_zp; Q.q[Q.n] = h->s_q; ++Q.n;
        }
    }
    if (!any) return EI_IMPULSE_OK;
    HIP_TRY(hipMemcpyAsync(b->d_lists, b->h_lists.data(), at[K] * sizeof(int), hipMemcpyHostToDevice, s));
    if (!b->lists_ev) HIP_TRY(hipEventCreateWithFlags(&b->lists_ev, hipEventDisableTiming));
    HIP_TRY(hipEventRecord(b->lists_ev, s));
    b->lists_ev_used = true;
    const int grid_cap = grid_cap_nn(b->m[0]);
    KWS_LAUNCH_TRY_OBJ("routed bank NN kernel", kws_launch_bank_nn_mfma_routed(b->d_rec, o16, l16, 16, feat, n16, grid_cap, s));
    KWS_LAUNCH_TRY_OBJ("routed bank NN kernel", kws_launch_bank_nn_mfma_routed(b->d_rec, o64, l64, 64, feat, n64, grid_cap, s));
    KWS_LAUNCH_TRY("routed bank quantise kernel", kws_launch_bank_quantize_routed(feat, (int)F, Q, lq, nq, s));
    for (size_t k = 0; k < K; ++k) {
        kws_handle *h = b->m[k];
        const int n = b->h_lists[at[k]];
        if (!scores[k] || n == 0 || !(h->is_float || !kws_nn_uses_mfma(h->nn))) continue;
        float *dst = scores[k] + row0 * h->model.labels.size();
        if ((e = network_device(h, feat, h->s_q, (size_t)n, dst, nullptr, nullptr, nullptr, nullptr, b->d_lists + at[k], s))) return e;
    }
    return EI_IMPULSE_OK;
}

// every member's network from the feature matrix feat [B][F] (device); scores[k] + row0 * labels of member k is where its rows go
EI_IMPULSE_ERROR bank_networks(kws_bank *b, const float *feat, size_t B, float *const *scores, size_t row0, hipStream_t s, const uint32_t *routes)
{
    // (routes that all name every member: the unrouted launches, which need no list)
    const uint32_t every = (1u << b->m.size()) - 1u;
    for (size_t i = 0; routes && i < B; ++i)
        if (routes[i] != every) return bank_networks_routed(b, feat, B, scores, row0, routes, s);
    const size_t K = b->m.size(), F = b->m[0]->model.nn_input_frame_size;
    KwsBankOut o16{}, o64{};
    KwsBankQuant Q{};
    EI_IMPULSE_ERROR e;
    for (size_t k = 0; k < K; ++k) {
        kws_handle *h = b->m[k];
        if (!scores[k] || h->is_float) continue;
        float *dst = scores[k] + row0 * h->model.labels.size();
        if (kws_nn_uses_mfma(h->nn)) {
            KwsBankOut &o = h->nn.blk[0].in_cpad == 16 ? o16 : o64;       // (kws_launch_nn's rule: 16-byte rows, or up to 64)
            o.rec[o.n] = (int)k; o.scores[o.n] = dst; ++o.n;
        } else {
            if ((e = ensure_scratch(h, B))) return e;
            Q.scale[Q.n] = h->nn.in_scale; Q.zp[Q.n] = h->nn.in_zp; Q.q[Q.n] = h->s_q; ++Q.n;
        }
    }
    const int grid_cap = grid_cap_nn(b->m[0]);
    KWS_LAUNCH_TRY_OBJ("bank NN kernel", kws_launch_bank_nn_mfma(b->d_rec, o16, 16, feat, (int)B, grid_cap, s));
    KWS_LAUNCH_TRY_OBJ("bank NN kernel", kws_launch_bank_nn_mfma(b->d_rec, o64, 64, feat, (int)B, grid_cap, s));
    KWS_LAUNCH_TRY("bank quantise kernel", kws_launch_bank_quantize(feat, B * F, Q, s));
    for (size_t k = 0; k < K; ++k) {
        kws_handle *h = b->m[k];
        if (!scores[k]) continue;
        float *dst = scores[k] + row0 * h->model.labels.size();
        if ((h->is_float || !kws_nn_uses_mfma(h->nn)) && (e = network_device(h, feat, h->s_q, B, dst, nullptr, nullptr, nullptr, nullptr, nullptr, s))) return e;
    }
    return EI_IMPULSE_OK;
}

bool bank_wants_nothing(const kws_bank *b, float *const *scores, const float *features)
{
    if (features) return false;
    for (size_t k = 0; k < b->m.size(); ++k) if (scores[k]) return false;
    return true;
}

// the finishing step of a chunk of gathered windows for a bank (the slide's, and the window pipelines' of kws_bank_windows.cpp): cmvnw (the MFE
// normalisation) once through the first member, then every member
EI_IMPULSE_ERROR bank_window_finish(void *ctx, float *win, size_t n, size_t g0, hipStream_t s)
{
    if (n == 0) return EI_IMPULSE_OK;
    BankWindows &c = *(BankWindows *)ctx;
    kws_bank *b = c.b;
    kws_handle *h0 = b->m[0];
    const size_t F = h0->model.nn_input_frame_size;
    EI_IMPULSE_ERROR e;
    float *f = c.features ? c.features + g0 * F : nullptr;
    if (!f) {
        if ((e = grow_buffer(&b->feat, &b->feat_cap, n * F))) return e;
        f = b->feat;
    }
    if ((e = cmvn_nn_device(h0, win, n, f, nullptr, nullptr, nullptr, nullptr, nullptr, s))) return e;
    return bank_networks(b, f, n, c.scores, g0, s, c.routes ? c.routes + g0 : nullptr);
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
    if (b->d_lists) (void)hipFree(b->d_lists);
    if (b->lists_ev) (void)hipEventDestroy(b->lists_ev);
    if (b->d_routes) (void)hipFree(b->d_routes);
    if (b->routes_ev) (void)hipEventDestroy(b->routes_ev);
    delete b;
}

size_t kws_bank_size(const kws_bank *b) { return b ? b->m.size() : 0; }
kws_handle *kws_bank_member(const kws_bank *b, size_t k) { return b && k < b->m.size() ? b->m[k] : nullptr; }

EI_IMPULSE_ERROR kws_bank_run_classifier_batch_device(kws_bank *b, const int16_t *pcm, size_t B, float *const *scores, float *features, void *stream)
{
    if (!b || !pcm || !scores) return fail(KWS_ERROR_BAD_ARGUMENT, "null argument");
    if (bank_wants_nothing(b, scores, features)) return fail(KWS_ERROR_BAD_ARGUMENT, "no output requested: every scores[k] and features are NULL");
    if (B > 0x7fffffff) return fail(KWS_ERROR_BAD_ARGUMENT, "batch too large");
    if (B == 0) return EI_IMPULSE_OK;
    HIP_TRY(hipSetDevice(b->device));
    hipStream_t s = (hipStream_t)stream;
    BankUse use(b, s, false);
    kws_handle *h0 = b->m[0];
    EI_IMPULSE_ERROR e;
    float *f = features;
    if (!f) {
        if ((e = grow_buffer(&b->feat, &b->feat_cap, B * (size_t)h0->model.nn_input_frame_size))) return e;
        f = b->feat;
    }
    if ((e = mfcc_fused_device(h0, pcm, 0, B, f, nullptr, s))) return e;
    return bank_networks(b, f, B, scores, 0, s);
}

EI_IMPULSE_ERROR kws_bank_run_classifier_routed_device(kws_bank *b, const int16_t *pcm, size_t B, const uint32_t *routes, float *const *scores, float *features,
                                                       void *stream)
{
    if (!routes) return kws_bank_run_classifier_batch_device(b, pcm, B, scores, features, stream);
    if (!b || !pcm || !scores) return fail(KWS_ERROR_BAD_ARGUMENT, "null argument");
    if (bank_wants_nothing(b, scores, features)) return fail(KWS_ERROR_BAD_ARGUMENT, "no output requested: every scores[k] and features are NULL");
    if (B > 0x7fffffff) return fail(KWS_ERROR_BAD_ARGUMENT, "batch too large");
    const size_t bad = kws_bank_route_check(routes, B, b->m.size());
    if (bad < B) return fail(KWS_ERROR_BAD_ARGUMENT, "clip %zu: route 0x%x names a member at or above the bank's %zu", bad, routes[bad], b->m.size());
    if (B == 0) return EI_IMPULSE_OK;
    HIP_TRY(hipSetDevice(b->device));
    hipStream_t s = (hipStream_t)stream;
    BankUse use(b, s, false);
    kws_handle *h0 = b->m[0];
    EI_IMPULSE_ERROR e;
    float *f = features;
    if (!f) {
        if ((e = grow_buffer(&b->feat, &b->feat_cap, B * (size_t)h0->model.nn_input_frame_size))) return e;
        f = b->feat;
    }
    if ((e = mfcc_fused_device(h0, pcm, 0, B, f, nullptr, s))) return e;
    return bank_networks(b, f, B, scores, 0, s, routes);
}

EI_IMPULSE_ERROR kws_bank_cmvn_inference_batch_device(kws_bank *b, const float *mfcc, size_t B, float *const *scores, float *features, void *stream)
{
    return kws_bank_cmvn_inference_routed_device(b, mfcc, B, nullptr, scores, features, stream);
}

EI_IMPULSE_ERROR kws_bank_cmvn_inference_routed_device(kws_bank *b, const float *mfcc, size_t B, const uint32_t *routes, float *const *scores, float *features, void *stream)
{
    if (!b || !mfcc || !scores) return fail(KWS_ERROR_BAD_ARGUMENT, "null argument");
    if (bank_wants_nothing(b, scores, features)) return fail(KWS_ERROR_BAD_ARGUMENT, "no output requested: every scores[k] and features are NULL");
    if (B > 0x7fffffff) return fail(KWS_ERROR_BAD_ARGUMENT, "batch too large");
    const size_t bad = routes ? kws_bank_route_check(routes, B, b->m.size()) : B;
    if (bad < B) return fail(KWS_ERROR_BAD_ARGUMENT, "row %zu: route 0x%x names a member at or above the bank's %zu", bad, routes[bad], b->m.size());
    if (B == 0) return EI_IMPULSE_OK;
    HIP_TRY(hipSetDevice(b->device));
    hipStream_t s = (hipStream_t)stream;
    BankUse use(b, s, false);
    kws_handle *h0 = b->m[0];
    EI_IMPULSE_ERROR e;
    float *f = features;
    if (!f) {
        if ((e = grow_buffer(&b->feat, &b->feat_cap, B * (size_t)h0->model.nn_input_frame_size))) return e;
        f = b->feat;
    }
    if ((e = ensure_scratch(h0, B))) return e;        // (a general-shape int8 first member: cmvn_nn_device writes its int8 tensor there)
    if ((e = cmvn_nn_device(h0, mfcc, B, f, nullptr, nullptr, nullptr, nullptr, nullptr, s))) return e;
    return bank_networks(b, f, B, scores, 0, s, routes);
}

EI_IMPULSE_ERROR kws_bank_slide_recordings_device(kws_bank *b, const int16_t *pcm, const size_t *offsets, const size_t *lengths, size_t R,
                                                  size_t hop_samples, int flags, float *const *scores, float *features, void *stream)
{
    if (!b || !scores) return fail(KWS_ERROR_BAD_ARGUMENT, "null argument");
    if (bank_wants_nothing(b, scores, features)) return fail(KWS_ERROR_BAD_ARGUMENT, "no output requested: every scores[k] and features are NULL");
    // the window count is any member's; the bound on windows x labels holds for the member with the most labels
    kws_slide_plan_info I;
    EI_IMPULSE_ERROR e;
    for (kws_handle *h : b->m)
        if ((e = kws_slide_plan(h, lengths, R, hop_samples, flags, &I))) return e;
    HIP_TRY(hipSetDevice(b->device));
    hipStream_t s = (hipStream_t)stream;
    BankUse use(b, s, true);
    BankWindows ctx{ b, scores, features };
    return kws_slide_run(b->m[0], pcm, offsets, lengths, R, hop_samples, flags, 0, bank_window_finish, &ctx, s);
}

#pragma GCC visibility pop
}
