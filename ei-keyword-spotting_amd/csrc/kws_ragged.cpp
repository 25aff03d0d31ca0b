// kws_ragged.cpp -- kws_run_classifier_ragged_device: run_classifier() for B clips of their own lengths (contract in include/kws/kws.h).
//
// The lengths are host data: every clip's frame count is worked out and checked here before anything is enqueued.  Then
//   MFCC block on the tuned shapes   ONE launch of kws_mfcc8_ragged_kernel over a table of per-clip descriptors (kws_ragged.h), whatever the
//                                    mix of lengths.  A clip whose first sample lies on a 16-byte boundary is read where it is; the others
//                                    are first copied into aligned slots of a staging buffer (kws_ragged_stage_kernel) -- the kernel's
//                                    16-byte loads need the alignment, and no load may reach outside the clip.
//   MFE block, general-shape plans   the grouped route: clips are bucketed by frame count; each bucket is gathered into slots of one stride
//                                    (with its wrap samples), run through the existing fixed-length launches with kws_plan_for_length's
//                                    plan, and its packed rows are scattered into the full-stride rows (kws_ragged_scatter_kernel).
// and the network is the existing launches on the [B][feature_count] matrix / int8 tensor -- a callable behind the DSP route (kws_ragged_run): a
// bank runs the route once with the network skipped, then every member's network on the feature rows (kws_bank_windows.cpp).
// These are the launches of KWS_MODE_EXACT: nothing here reads the handle's mode, its fast counters or its logits tap.
#include "kws_internal.h"
#include "kws_ragged.h"

#include <algorithm>

struct KwsRaggedScratch {
    KwsRaggedClip *clips = nullptr, *list = nullptr;    // the kernel's table [B]; the staging / gather list
    int16_t *stage = nullptr;
    float *wrap = nullptr, *packed = nullptr;
    const int *pad_maps = nullptr;                      // [frames + 1][map_stride], uploaded once (in the handle's dev_allocs)
    int map_stride = 0;
    size_t clips_cap = 0, list_cap = 0, stage_cap = 0, wrap_cap = 0, packed_cap = 0;
    std::vector<KwsRaggedClip> h_clips, h_list;         // host copies, kept for their capacity
};

static const size_t kStageSlack = 64;        // samples behind the last slot: the fixed-length kernels fetch whole 16-byte groups

static void ragged_release(kws_handle *h)
{
    KwsRaggedScratch *s = h->ragged;
    if (!s) return;
    for (void *p : { (void *)s->clips, (void *)s->list, (void *)s->stage, (void *)s->wrap, (void *)s->packed })
        if (p) (void)hipFree(p);
    delete s;
    h->ragged = nullptr;
}

#pragma GCC visibility push(default)     // the C ABI
int kws_window_frame_count(const kws_handle *h, size_t n_samples) { return h ? kws_frames_for_length(h, n_samples) : 0; }
#pragma GCC visibility pop

static EI_IMPULSE_ERROR ragged_pad_maps(kws_handle *h, KwsRaggedScratch &S)
{
    if (S.pad_maps) return EI_IMPULSE_OK;
    const int nf = h->dsp.n_frames, stride = nf + 2 * h->dsp.pad;
    std::vector<int> all((size_t)(nf + 1) * stride, 0), one;
    for (int r = 1; r <= nf; ++r) {
        h_pad_map(r, h->dsp.pad, one);
        std::copy(one.begin(), one.end(), all.begin() + (size_t)r * stride);
    }
    if (EI_IMPULSE_ERROR e = h->upload(all, &S.pad_maps)) return e;
    S.map_stride = stride;
    return EI_IMPULSE_OK;
}

// the tuned shapes: one DSP launch
static EI_IMPULSE_ERROR ragged_tuned(kws_handle *h, KwsRaggedScratch &S, const int16_t *pcm, const size_t *offsets, const size_t *lengths, size_t B,
                                     float *f, int8_t *q, hipStream_t s)
{
    EI_IMPULSE_ERROR e;
    S.h_clips.resize(B);
    S.h_list.clear();
    size_t slot = 0;
    for (size_t i = 0; i < B; ++i) {
        const int16_t *x = pcm + offsets[i];
        S.h_clips[i] = { x, (int)lengths[i], kws_frames_for_length(h, lengths[i]) };
        if (((uintptr_t)x & 15) != 0) {
            S.h_list.push_back({ x, (int)lengths[i], 0 });
            slot = std::max(slot, (lengths[i] + 7) & ~(size_t)7);
        }
    }
    const size_t n_staged = S.h_list.size();
    if ((e = ragged_pad_maps(h, S)) || (e = grow_buffer(&S.clips, &S.clips_cap, B)) || (e = grow_buffer(&S.list, &S.list_cap, n_staged)) ||
        (e = grow_buffer(&S.stage, &S.stage_cap, n_staged ? n_staged * slot + kStageSlack : 0)))
        return e;
    if (n_staged) {
        size_t j = 0;
        for (size_t i = 0; i < B; ++i)
            if (((uintptr_t)S.h_clips[i].x & 15) != 0) S.h_clips[i].x = S.stage + (j++) * slot;
        HIP_TRY(hipMemcpyAsync(S.list, S.h_list.data(), n_staged * sizeof(KwsRaggedClip), hipMemcpyHostToDevice, s));
        KWS_LAUNCH_TRY("staging kernel", kws_launch_ragged_stage(S.list, (int)n_staged, S.stage, (int)slot, nullptr, s));
    }
    HIP_TRY(hipMemcpyAsync(S.clips, S.h_clips.data(), B * sizeof(KwsRaggedClip), hipMemcpyHostToDevice, s));
    const KwsRaggedArgs R = { S.clips, S.pad_maps, S.map_stride };
    KWS_LAUNCH_TRY_OBJ("ragged MFCC kernel", kws_launch_mfcc_ragged(h->dsp, R, (int)B, f, q, h->nn.in_scale, h->nn.in_zp, (int)h->model.nn_input_frame_size, grid_cap_mfcc(h), s));
    return EI_IMPULSE_OK;
}

// MFE blocks and general-shape plans: one existing launch sequence per distinct frame count
static EI_IMPULSE_ERROR ragged_grouped(kws_handle *h, KwsRaggedScratch &S, const int16_t *pcm, const size_t *offsets, const size_t *lengths, size_t B,
                                       float *f, int8_t *q, hipStream_t s)
{
    EI_IMPULSE_ERROR e;
    const bool mfe = h->model.dsp.block == DSP_BLOCK_MFE;
    const int nf = h->dsp.n_frames, cols = mfe ? h->dsp.n_filters : h->dsp.n_cepstral;
    const size_t F = h->model.nn_input_frame_size;
    // counting sort by frame count: the list holds the clips bucket after bucket, each with its row of the outputs
    std::vector<size_t> first(nf + 2, 0), slot(nf + 1, 0), rep(nf + 1, 0);
    std::vector<int> fr(B);
    for (size_t i = 0; i < B; ++i) {
        fr[i] = kws_frames_for_length(h, lengths[i]);
        ++first[fr[i] + 1];
        slot[fr[i]] = std::max(slot[fr[i]], (lengths[i] + 7) & ~(size_t)7);
        rep[fr[i]] = lengths[i];
    }
    for (int r = 1; r <= nf + 1; ++r) first[r] += first[r - 1];
    S.h_list.resize(B);
    {
        std::vector<size_t> at(first.begin(), first.end() - 1);
        for (size_t i = 0; i < B; ++i) S.h_list[at[fr[i]]++] = { pcm + offsets[i], (int)lengths[i], (int)i };
    }
    size_t stage_need = 0, packed_need = 0, wrap_need = 0;
    for (int r = 1; r <= nf; ++r) {
        const size_t n = first[r + 1] - first[r];
        stage_need = std::max(stage_need, n * slot[r]);
        packed_need = std::max(packed_need, n * (size_t)r * cols);
        wrap_need = std::max(wrap_need, n);
    }
    if ((e = grow_buffer(&S.list, &S.list_cap, B)) || (e = grow_buffer(&S.stage, &S.stage_cap, stage_need + kStageSlack)) ||
        (e = grow_buffer(&S.packed, &S.packed_cap, packed_need)) || (e = grow_buffer(&S.wrap, &S.wrap_cap, wrap_need)))
        return e;
    HIP_TRY(hipMemcpyAsync(S.list, S.h_list.data(), B * sizeof(KwsRaggedClip), hipMemcpyHostToDevice, s));
    for (int r = 1; r <= nf; ++r) {
        const size_t n = first[r + 1] - first[r];
        if (!n) continue;
        KwsDspPlan P;
        if ((e = kws_plan_for_length(h, rep[r], &P))) return e;
        P.n_samples = (int)slot[r];               // the slots' stride; the wrap sample is handed over per clip
        const KwsRaggedClip *list = S.list + first[r];
        KWS_LAUNCH_TRY("gather kernel", kws_launch_ragged_stage(list, (int)n, S.stage, (int)slot[r], S.wrap, s));
        if (mfe) {
            // (no pre-emphasis in front of feature::mfe: no wrap sample)
            if ((e = mfcc_fused_device_plan(h, P, S.stage, 0, n, S.packed, nullptr, s))) return e;
        } else {
            kws_handle::GenericBuf *g = nullptr;
            if ((e = generic_for(h, s, n, &g)) || (e = spectral_device(h, P, S.stage, 0, n, g->mfcc, S.wrap, s, 0))) return e;
            KWS_LAUNCH_TRY("cmvnw kernel", kws_launch_cmvn_generic(P, g->mfcc, (int)n, S.packed, nullptr, h->nn.in_scale, h->nn.in_zp, s));
        }
        KWS_LAUNCH_TRY("scatter kernel", kws_launch_ragged_scatter(S.packed, list, (int)n, r * cols, (int)F, f, q, h->nn.in_scale, h->nn.in_zp, s));
    }
    return EI_IMPULSE_OK;
}

// The network step of kws_run_classifier_ragged_device itself: the existing launches on the matrix / the int8 tensor the DSP route wrote
struct RaggedOwn {
    kws_handle *h;
    float *scores;
    int8_t *q_in;
};
static EI_IMPULSE_ERROR ragged_own_finish(void *ctx, float *f, size_t B, size_t, hipStream_t s)
{
    RaggedOwn &o = *(RaggedOwn *)ctx;
    kws_handle *h = o.h;
    if (!o.scores) return EI_IMPULSE_OK;
    const int8_t *q = h->is_float ? nullptr : o.q_in ? o.q_in : h->s_q;        // (the tensor kws_ragged_run had the DSP route write)
    return network_device(h, f, q, B, o.scores, nullptr, nullptr, nullptr, nullptr, nullptr, s);
}

// The ragged call up to the network: argument checks, then the DSP route into f [B][feature_count] and the int8 tensor q, then
// finish(ctx, f, B, 0, s) once (kws_internal.h has the contract; `me` names the public call in messages).
EI_IMPULSE_ERROR kws_ragged_run(kws_handle *h, const int16_t *pcm, const size_t *offsets, const size_t *lengths, size_t B, float *features, int8_t *q_in,
                                int net, int take_lock, kws_slide_finish_fn finish, void *ctx, hipStream_t s)
{
    static const char *const me = "kws_run_classifier_ragged_device";
    if (!h) return fail(KWS_ERROR_BAD_ARGUMENT, "%s: null handle", me);
    if (B >= ((size_t)1 << 31)) return fail(KWS_ERROR_BAD_ARGUMENT, "%s: batch too large (%zu clips)", me, B);
    if (!net && !features && !q_in) return fail(KWS_ERROR_BAD_ARGUMENT, "%s: no output requested (scores, features and q_in are all NULL)", me);
    if (h->is_float && q_in) return fail(KWS_ERROR_UNSUPPORTED_MODEL, "int8 input tensor requested from a float32 model");
    if (B == 0) return EI_IMPULSE_OK;
    if (!pcm || !offsets || !lengths) return fail(KWS_ERROR_BAD_ARGUMENT, "%s: null %s", me, !pcm ? "pcm" : !offsets ? "offsets" : "lengths");
    for (size_t i = 0; i < B; ++i) {
        const int nfr = kws_frames_for_length(h, lengths[i]);
        if (nfr < 1 || nfr > h->dsp.n_frames)
            return fail(KWS_ERROR_BAD_ARGUMENT, "%s: clip %zu has %zu samples, %d frames: a clip needs 1 .. %d (longer audio: kws_slide_recordings_device)", me, i,
                        lengths[i], nfr, h->dsp.n_frames);
    }
    HIP_TRY(hipSetDevice(h->device));
    std::unique_lock<std::mutex> lk(h->mu, std::defer_lock);
    if (take_lock) lk.lock();
    if (!h->ragged) { h->ragged = new KwsRaggedScratch(); h->ragged_release = ragged_release; }
    KwsRaggedScratch &S = *h->ragged;
    EI_IMPULSE_ERROR e = ensure_scratch(h, B);
    if (e) return e;
    ScratchUse use(h, s);
    // what the handle's network reads when the caller does not ask for it: the handle's scratch
    float *f = (features || !(net && h->is_float)) ? features : h->s_mfcc;
    int8_t *q = h->is_float ? nullptr : (q_in || !net) ? q_in : h->s_q;
    const bool tuned = h->model.dsp.block == DSP_BLOCK_MFCC && kws_mfcc_ragged_serves(h->dsp);
    e = tuned ? ragged_tuned(h, S, pcm, offsets, lengths, B, f, q, s) : ragged_grouped(h, S, pcm, offsets, lengths, B, f, q, s);
    if (e) return e;
    return finish(ctx, f, B, 0, s);
}

#pragma GCC visibility push(default)
EI_IMPULSE_ERROR kws_run_classifier_ragged_device(kws_handle *h, const int16_t *pcm, const size_t *offsets, const size_t *lengths, size_t B,
                                                  float *scores, float *features, int8_t *q_in, void *stream)
{
    RaggedOwn own{ h, scores, q_in };
    return kws_ragged_run(h, pcm, offsets, lengths, B, features, q_in, scores != nullptr, 1, ragged_own_finish, &own, (hipStream_t)stream);
}
#pragma GCC visibility pop
