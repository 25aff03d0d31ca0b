// ragged_host_driver.cpp -- TEST INFRASTRUCTURE ONLY (tests/test_ragged_host.py): the host side of kws_run_classifier_ragged_device -- the
// frame count, the refusals, the descriptor table, staging and grouping, scratch growth -- run against the launch-recording stub HIP
// runtime of ragged_hip_stub.cpp (device memory = host heap, launches do nothing) under ASan + UBSan.  No value a kernel would write
// means anything here.
// usage: kws_ragged_san l476 l476_f32 mfcc40 mfe general      prints
//   load <n> <code>
//   frames <n> <count for 0> <count for 1> ... <count for 17000>          models 0 and 4
//   refuse <model> <name> <code> <launches> <untouched: 1/0> <kws_last_error text>
//   ok <model> <name> <code> <launches> <untouched: 1/0>                  calls that succeed and must write and launch nothing
//   call <model> <name> <code>
//   launches <model> <name> <dsp launches> <ragged kernel launches> <all launches>
//   done
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../include/kws/kws.h"

extern "C" void kws_stub_launch_reset(void);
extern "C" int kws_stub_launch_count(const char *substring);

static int dsp_launches() { return kws_stub_launch_count("") - kws_stub_launch_count("kws_nn"); }

struct Bufs {
    std::vector<float> s, f;
    std::vector<int8_t> q;
    Bufs(size_t B, kws_handle *h) : s(B * (size_t)kws_label_count(h) + 1, -7.0f), f(B * (size_t)kws_feature_count(h) + 1, -7.0f), q(B * (size_t)kws_feature_count(h) + 1, 77) {}
    int untouched() const
    {
        for (float v : s) if (v != -7.0f) return 0;
        for (float v : f) if (v != -7.0f) return 0;
        for (int8_t v : q) if (v != 77) return 0;
        return 1;
    }
};

// lengths: shortest .. longest valid, spread by a fixed rule; offsets back to back (mostly unaligned) or on 16-byte boundaries
static void layout(kws_handle *h, size_t B, bool aligned, int distinct, std::vector<size_t> &off, std::vector<size_t> &len, size_t *total)
{
    const size_t clip = (size_t)kws_clip_samples(h);
    size_t lo = 0, hi = clip;
    while (kws_window_frame_count(h, lo) < 1) ++lo;
    while (kws_window_frame_count(h, hi + 1) == kws_frame_count(h)) ++hi;
    off.resize(B); len.resize(B);
    size_t at = 0;
    for (size_t i = 0; i < B; i++) {
        len[i] = distinct <= 1 ? clip : lo + ((i * 2654435761u) % (size_t)distinct) * (hi - lo) / (size_t)(distinct - 1);
        if (aligned) at = (at + 7) & ~(size_t)7;
        off[i] = at;
        at += len[i];
    }
    *total = at + 8;
}

static void exercise(int mi, kws_handle *h, bool is_float)
{
    const size_t clip = (size_t)kws_clip_samples(h);
    const int nf = kws_frame_count(h);
    std::vector<size_t> off, len;
    size_t total = 0;
    layout(h, 7, false, 7, off, len, &total);
    std::vector<int16_t> pcm(total, 3);
    // ---- refusals: the code, the text, no launch, nothing written
    auto refuse = [&](const char *name, kws_handle *hh, const int16_t *p, const size_t *o, const size_t *l, size_t B, bool s, bool f, bool q) {
        Bufs b(7, h);
        kws_stub_launch_reset();
        EI_IMPULSE_ERROR rc = kws_run_classifier_ragged_device(hh, p, o, l, B, s ? b.s.data() : nullptr, f ? b.f.data() : nullptr, q ? b.q.data() : nullptr, nullptr);
        printf("%s %d %s %d %d %d %s\n", rc ? "refuse" : "ok", mi, name, (int)rc, kws_stub_launch_count(""), b.untouched(), rc ? kws_last_error() : "");
    };
    size_t lo = len[0], hi = len[0];
    for (size_t v : len) { lo = v < lo ? v : lo; hi = v > hi ? v : hi; }
    for (int k = 0; k < 3; k++) {
        std::vector<size_t> bad(len);
        bad[3] = k == 0 ? 0 : k == 1 ? lo - 1 : hi + 1;
        refuse(k == 0 ? "len0_at3" : k == 1 ? "short_at3" : "long_at3", h, pcm.data(), off.data(), bad.data(), 7, true, true, !is_float);
    }
    {
        std::vector<size_t> bad(len);
        bad[5] = 1; bad[6] = 0;
        refuse("first_of_two_at5", h, pcm.data(), off.data(), bad.data(), 7, true, false, false);
    }
    refuse("all_null", h, pcm.data(), off.data(), len.data(), 7, false, false, false);
    refuse("null_handle", nullptr, pcm.data(), off.data(), len.data(), 7, true, false, false);
    refuse("null_pcm", h, nullptr, off.data(), len.data(), 7, true, false, false);
    refuse("null_offsets", h, pcm.data(), nullptr, len.data(), 7, true, false, false);
    refuse("null_lengths", h, pcm.data(), off.data(), nullptr, 7, true, false, false);
    refuse("huge_batch", h, pcm.data(), off.data(), len.data(), (size_t)1 << 31, true, false, false);
    if (is_float) refuse("q_on_float", h, pcm.data(), off.data(), len.data(), 7, true, false, true);
    refuse("b0", h, pcm.data(), off.data(), len.data(), 0, true, true, !is_float);
    refuse("b0_null_arrays", h, nullptr, nullptr, nullptr, 0, true, false, false);
    // ---- batch sizes and scratch: growth and reuse across calls of different sizes, staged and in place
    const struct { const char *name; size_t B; bool aligned; int distinct; bool s, f, q; } calls[] = {
        { "b1", 1, true, 1, true, true, true },          { "b10_staged", 10, false, 10, true, false, false },
        { "b5000_mixed", 5000, false, 4999, true, true, true }, { "b3_reuse", 3, false, 3, true, false, false },
        { "b7000_aligned", 7000, true, nf, true, false, false }, { "b64_features_only", 64, false, 64, false, true, false },
        { "b64_q_only", 64, true, 64, false, false, true },
    };
    for (const auto &c : calls) {
        if (c.q && is_float && !c.s && !c.f) continue;
        layout(h, c.B, c.aligned, c.distinct, off, len, &total);
        std::vector<int16_t> p(total, 5);
        Bufs b(c.B, h);
        EI_IMPULSE_ERROR rc = kws_run_classifier_ragged_device(h, p.data(), off.data(), len.data(), c.B, c.s ? b.s.data() : nullptr, c.f ? b.f.data() : nullptr,
                                                               (c.q && !is_float) ? b.q.data() : nullptr, nullptr);
        printf("call %d %s %d\n", mi, c.name, (int)rc);
    }
    // ---- launches: one distinct length against every frame count, clips on 16-byte boundaries (read in place), then back to back (staged)
    const struct { const char *name; bool aligned; int distinct; } ls[] = { { "one_length", true, 1 }, { "all_frame_counts", true, nf },
                                                                             { "all_frame_counts_staged", false, nf } };
    for (const auto &c : ls) {
        layout(h, 490, c.aligned, c.distinct, off, len, &total);
        std::vector<int16_t> p(total, 5);
        Bufs b(490, h);
        kws_stub_launch_reset();
        EI_IMPULSE_ERROR rc = kws_run_classifier_ragged_device(h, p.data(), off.data(), len.data(), 490, b.s.data(), nullptr, nullptr, nullptr);
        printf("launches %d %s %d %d %d\n", mi, c.name, rc ? -1 : dsp_launches(), kws_stub_launch_count("kws_mfcc8_ragged_kernel"), kws_stub_launch_count(""));
    }
    (void)clip;
}

int main(int argc, char **argv)
{
    std::vector<kws_handle *> hs;
    for (int i = 1; i < argc; i++) {
        kws_handle *h = nullptr;
        EI_IMPULSE_ERROR rc = kws_create_from_file(argv[i], 0, &h);
        printf("load %d %d\n", i - 1, (int)rc);
        if (rc) return 1;
        hs.push_back(h);
    }
    if (hs.size() != 5) return 2;
    const int which[2] = { 0, 4 };
    for (int w : which) {
        printf("frames %d", w);
        for (size_t n = 0; n <= 17000; n++) printf(" %d", kws_window_frame_count(hs[w], n));
        printf("\n");
    }
    printf("frames_null %d\n", kws_window_frame_count(nullptr, 16000));
    for (size_t i = 0; i < hs.size(); i++) exercise((int)i, hs[i], kws_model_is_float(hs[i]) != 0);
    for (kws_handle *h : hs) kws_destroy(h);
    printf("done\n");
    return 0;
}
