// bank_windows_host_driver.cpp -- TEST INFRASTRUCTURE ONLY (tests/test_bank_windows_host.py): argument checks, counts and the host
// bookkeeping of the banks' window pipelines (kws_bank_scan_recordings_device, kws_bank_live_*, kws_bank_slide_live_*,
// kws_bank_run_classifier_ragged_device) run against the stub HIP runtime of tests/sanitize (device memory = host heap, launches do nothing)
// under ASan + UBSan.  No value a kernel would write means anything here.  With KWS_STUB_RECORD set the stub records every launch; the
// driver brackets each call it wants counted with "BEGIN <bank> <name>" / "END" notes.
// usage: kws_bank_windows_san mfcc40_a mfcc40_b mfcc40_c mfcc40_d l476 l476_f32 l432      prints
//   load <n> <code>
//   refuse <bank> <name> <code> <outputs and session state untouched: 1/0>      (recorded: must launch nothing)
//   empty <bank> <name> <code> <untouched>                                      (recorded: must launch nothing)
//   call <bank> <name> <code>                                                   (recorded)
//   counts <bank> <name> <pushes or calls> <mismatches against the single-model functions>
//   done
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../include/kws/kws.h"

extern "C" void kws_stub_note(const char *line);

static const float FILL = -7.0f;

static bool all_are(const std::vector<float> &v, float x)
{
    for (float f : v) if (f != x) return false;
    return true;
}

struct Section {
    Section(const char *bank, const char *name) { kws_stub_note((std::string("BEGIN ") + bank + " " + name).c_str()); }
    ~Section() { kws_stub_note("END"); }
};

struct Outputs {
    std::vector<std::vector<float>> sc, raw;
    std::vector<float *> sp, rp, none;
    std::vector<float> feats;
    Outputs(kws_bank *b, size_t rows)
    {
        const size_t K = kws_bank_size(b);
        sc.resize(K); raw.resize(K); sp.resize(K); rp.resize(K); none.assign(K, nullptr);
        for (size_t k = 0; k < K; k++) {
            const size_t C = (size_t)kws_label_count(kws_bank_member(b, k));
            sc[k].assign(rows * C, FILL); raw[k].assign(rows * C, FILL);
            sp[k] = sc[k].data(); rp[k] = raw[k].data();
        }
        feats.assign(rows * (size_t)kws_feature_count(kws_bank_member(b, 0)), FILL);
    }
    int untouched() const
    {
        bool ok = all_are(feats, FILL);
        for (size_t k = 0; k < sc.size(); k++) ok = ok && all_are(sc[k], FILL) && all_are(raw[k], FILL);
        return ok ? 1 : 0;
    }
};

static unsigned rnd(unsigned &s) { s = s * 1664525u + 1013904223u; return s >> 8; }

static void exercise(const char *name, kws_bank *b)
{
    const size_t K = kws_bank_size(b);
    kws_handle *h0 = kws_bank_member(b, 0);
    const size_t clip = (size_t)kws_clip_samples(h0), stride = (size_t)kws_frame_stride_samples(h0), slice = 4000, S = 5;
    std::vector<int16_t> pcm(400000, 3);
    Outputs o(b, 256);
    EI_IMPULSE_ERROR rc;
    auto refuse = [&](const char *what, EI_IMPULSE_ERROR code, int state_ok = 1) { printf("refuse %s %s %d %d\n", name, what, (int)code, o.untouched() && state_ok); };

    // ---- the scan
    const size_t off3[3] = { 1, 50001, 100003 }, len3[3] = { 15999, 16000 + 3999, 40000 };
    { Section s(name, "scan_null_bank"); refuse("scan_null_bank", kws_bank_scan_recordings_device(nullptr, pcm.data(), off3, len3, 3, slice, o.sp.data(), nullptr, nullptr)); }
    { Section s(name, "scan_null_scores"); refuse("scan_null_scores", kws_bank_scan_recordings_device(b, pcm.data(), off3, len3, 3, slice, nullptr, o.rp.data(), nullptr)); }
    { Section s(name, "scan_nothing_wanted"); refuse("scan_nothing_wanted", kws_bank_scan_recordings_device(b, pcm.data(), off3, len3, 3, slice, o.none.data(), o.rp.data(), nullptr)); }
    { Section s(name, "scan_bad_slicing"); refuse("scan_bad_slicing", kws_bank_scan_recordings_device(b, pcm.data(), off3, len3, 3, 4001, o.sp.data(), nullptr, nullptr)); }
    { Section s(name, "scan_null_pcm"); refuse("scan_null_pcm", kws_bank_scan_recordings_device(b, nullptr, off3, len3, 3, slice, o.sp.data(), nullptr, nullptr)); }
    { Section s(name, "scan_r0"); rc = kws_bank_scan_recordings_device(b, pcm.data(), nullptr, nullptr, 0, slice, o.sp.data(), o.rp.data(), nullptr); printf("empty %s scan_r0 %d %d\n", name, (int)rc, o.untouched()); }
    { Section s(name, "scan_short"); rc = kws_bank_scan_recordings_device(b, pcm.data(), off3, len3, 1, slice, o.sp.data(), o.rp.data(), nullptr); printf("empty %s scan_short %d %d\n", name, (int)rc, o.untouched()); }
    {
        // window counts are any member's; the bank call and member 0's own call on the same recordings, recorded for their launches
        size_t mism = 0, total = 0;
        for (size_t r = 0; r < 3; r++) {
            size_t w0 = 0;
            (void)kws_scan_window_count(h0, len3[r], slice, &w0);
            total += w0;
            for (size_t k = 1; k < K; k++) {
                size_t w = 0;
                (void)kws_scan_window_count(kws_bank_member(b, k), len3[r], slice, &w);
                mism += w != w0;
            }
        }
        printf("counts %s scan %zu %zu\n", name, total, mism);
        Outputs w(b, total + 2);
        { Section s(name, "scan"); printf("call %s scan %d\n", name, (int)kws_bank_scan_recordings_device(b, pcm.data(), off3, len3, 3, slice, w.sp.data(), w.rp.data(), nullptr)); }
        { Section s(name, "scan_in_place"); printf("call %s scan_in_place %d\n", name, (int)kws_bank_scan_recordings_device(b, pcm.data(), off3, len3, 3, slice, w.sp.data(), nullptr, nullptr)); }
        if (K > 1) {
            std::vector<float *> some(w.sp);
            some[0] = nullptr;
            Section s(name, "scan_skip0");
            printf("call %s scan_skip0 %d\n", name, (int)kws_bank_scan_recordings_device(b, pcm.data(), off3, len3, 3, slice, some.data(), w.rp.data(), nullptr));
        }
        { Section s(name, "scan_single"); printf("call %s scan_single %d\n", name, (int)kws_scan_recordings_device(h0, pcm.data(), off3, len3, 3, slice, w.sp[0], w.rp[0], nullptr)); }
    }

    // ---- live continuous sessions
    kws_bank_live *lv = (kws_bank_live *)(uintptr_t)0x10;
    { Section s(name, "live_create_slicing"); rc = kws_bank_live_create(b, S, 4001, &lv); refuse("live_create_slicing", rc, lv == nullptr); }
    { Section s(name, "live_create_s0"); rc = kws_bank_live_create(b, 0, slice, &lv); refuse("live_create_s0", rc, lv == nullptr); }
    { Section s(name, "live_create_null_bank"); rc = kws_bank_live_create(nullptr, S, slice, &lv); refuse("live_create_null_bank", rc, lv == nullptr); }
    kws_live *own = nullptr;
    if (kws_bank_live_create(b, S, slice, &lv) != EI_IMPULSE_OK || kws_live_create(h0, S, slice, &own) != EI_IMPULSE_OK) { printf("call %s live_create -1\n", name); return; }
    printf("call %s live_create 0\n", name);
    {
        // seeded random pushes to random subsets, finishes included: every count against the single-model session fed the same pushes
        unsigned seed = 12345;
        size_t pushes = 0, mism = 0;
        std::vector<size_t> streams, offs, lens, nb, ns;
        std::vector<int> fin;
        Outputs w(b, 64);
        for (int it = 0; it < 120; it++) {
            streams.clear(); offs.clear(); lens.clear(); fin.clear();
            for (size_t st = 0; st < S; st++) {
                if (rnd(seed) % 3 == 0) continue;
                const unsigned kind = rnd(seed) % 6;
                const size_t n = kind == 0 ? 0 : kind == 1 ? 1 : kind == 2 ? slice - 1 : kind == 3 ? slice : kind == 4 ? slice + 320 - (rnd(seed) & 1) : rnd(seed) % 30000;
                streams.push_back(st); offs.push_back(1 + 2 * (rnd(seed) % 1000)); lens.push_back(n); fin.push_back(rnd(seed) % 7 == 0);
            }
            const size_t n = streams.size();
            nb.assign(n, 99); ns.assign(n, 98);
            for (size_t i = 0; i < n; i++) {
                size_t a = 0, c = 1;
                (void)kws_bank_live_window_count(lv, streams[i], lens[i], fin[i], &a);
                (void)kws_live_window_count(own, streams[i], lens[i], fin[i], &c);
                mism += a != c;
            }
            if (it == 60) { const size_t two[2] = { 1, 3 }; mism += kws_bank_live_reset(lv, two, 2) != EI_IMPULSE_OK || kws_live_reset(own, two, 2) != EI_IMPULSE_OK; }
            const EI_IMPULSE_ERROR rb = kws_bank_live_push_device(lv, n, streams.data(), pcm.data(), offs.data(), lens.data(), fin.data(), w.sp.data(), w.rp.data(), nb.data(), nullptr);
            const EI_IMPULSE_ERROR rs = kws_live_push_device(own, n, streams.data(), pcm.data(), offs.data(), lens.data(), fin.data(), w.sp[0], w.rp[0], ns.data(), nullptr);
            mism += rb != EI_IMPULSE_OK || rs != EI_IMPULSE_OK;
            for (size_t i = 0; i < n; i++) mism += nb[i] != ns[i];
            pushes++;
        }
        printf("counts %s live %zu %zu\n", name, pushes, mism);
    }
    {
        const size_t st2[2] = { 0, 2 }, of2[2] = { 3, 70001 }, ln2[2] = { 3 * slice + 320, 6 * slice + 320 }, tw[2] = { 2, 2 }, far[2] = { 0, S };
        size_t nw[2] = { 77, 77 }, before[2], after[2];
        (void)kws_bank_live_reset(lv, nullptr, 0);
        (void)kws_live_reset(own, nullptr, 0);
        auto mirrors = [&](size_t *out) { for (int i = 0; i < 2; i++) (void)kws_bank_live_window_count(lv, st2[i], ln2[i], 0, &out[i]); };
        // a first push so that the streams have state a refusal could damage
        Outputs w(b, 64);
        { Section s(name, "live_push"); printf("call %s live_push %d\n", name, (int)kws_bank_live_push_device(lv, 2, st2, pcm.data(), of2, ln2, nullptr, w.sp.data(), w.rp.data(), nw, nullptr)); }
        { Section s(name, "live_push_single"); printf("call %s live_push_single %d\n", name, (int)kws_live_push_device(own, 2, st2, pcm.data(), of2, ln2, nullptr, w.sp[0], w.rp[0], nw, nullptr)); }
        mirrors(before);
        std::vector<float *> some(o.sp);
        some[K - 1] = nullptr;
        nw[0] = nw[1] = 77;
        auto same = [&]() { mirrors(after); return after[0] == before[0] && after[1] == before[1] && nw[0] == 77 && nw[1] == 77 ? 1 : 0; };
        { Section s(name, "live_push_null_member"); rc = kws_bank_live_push_device(lv, 2, st2, pcm.data(), of2, ln2, nullptr, some.data(), o.rp.data(), nw, nullptr); refuse("live_push_null_member", rc, same()); }
        { Section s(name, "live_push_null_scores"); rc = kws_bank_live_push_device(lv, 2, st2, pcm.data(), of2, ln2, nullptr, nullptr, o.rp.data(), nw, nullptr); refuse("live_push_null_scores", rc, same()); }
        { Section s(name, "live_push_twice"); rc = kws_bank_live_push_device(lv, 2, tw, pcm.data(), of2, ln2, nullptr, o.sp.data(), o.rp.data(), nw, nullptr); refuse("live_push_twice", rc, same()); }
        { Section s(name, "live_push_range"); rc = kws_bank_live_push_device(lv, 2, far, pcm.data(), of2, ln2, nullptr, o.sp.data(), o.rp.data(), nw, nullptr); refuse("live_push_range", rc, same()); }
        { Section s(name, "live_push_null_counts"); rc = kws_bank_live_push_device(lv, 2, st2, pcm.data(), of2, ln2, nullptr, o.sp.data(), o.rp.data(), nullptr, nullptr); refuse("live_push_null_counts", rc, same()); }
        { Section s(name, "live_push_null_session"); rc = kws_bank_live_push_device(nullptr, 2, st2, pcm.data(), of2, ln2, nullptr, o.sp.data(), o.rp.data(), nw, nullptr); refuse("live_push_null_session", rc, same()); }
        { Section s(name, "live_reset_range"); rc = kws_bank_live_reset(lv, far, 2); refuse("live_reset_range", rc, same()); }
        const size_t zero[2] = { 0, 0 };
        { Section s(name, "live_push_n0"); rc = kws_bank_live_push_device(lv, 0, nullptr, nullptr, nullptr, nullptr, nullptr, o.sp.data(), nullptr, nullptr, nullptr); printf("empty %s live_push_n0 %d %d\n", name, (int)rc, o.untouched() && same()); }
        { Section s(name, "live_push_zero_lengths"); rc = kws_bank_live_push_device(lv, 2, st2, nullptr, nullptr, zero, nullptr, o.sp.data(), o.rp.data(), nw, nullptr); printf("empty %s live_push_zero_lengths %d %d\n", name, (int)rc, o.untouched() && nw[0] == 0 && nw[1] == 0); }
    }

    // ---- live one-shot windows
    kws_bank_slide_live *sl = (kws_bank_slide_live *)(uintptr_t)0x10;
    { Section s(name, "slide_create_hop0"); rc = kws_bank_slide_live_create(b, S, 0, 0, &sl); refuse("slide_create_hop0", rc, sl == nullptr); }
    { Section s(name, "slide_create_flags"); rc = kws_bank_slide_live_create(b, S, 5 * stride, 3, &sl); refuse("slide_create_flags", rc, sl == nullptr); }
    { Section s(name, "slide_create_unserved"); rc = kws_bank_slide_live_create(b, S, 1000, KWS_SLIDE_SHARED, &sl); refuse("slide_create_unserved", rc, sl == nullptr); }
    { Section s(name, "slide_create_null_bank"); rc = kws_bank_slide_live_create(nullptr, S, 5 * stride, 0, &sl); refuse("slide_create_null_bank", rc, sl == nullptr); }
    kws_bank_slide_live *sessions[3] = { nullptr, nullptr, nullptr };
    const size_t hops[3] = { 5 * stride, 1000, 5 * stride };
    const int flags[3] = { KWS_SLIDE_AUTO, KWS_SLIDE_AUTO, KWS_SLIDE_DIRECT };
    for (int q = 0; q < 3; q++) {
        kws_slide_live *sown = nullptr;
        if (kws_bank_slide_live_create(b, S, hops[q], flags[q], &sessions[q]) != EI_IMPULSE_OK || kws_slide_live_create(h0, S, hops[q], flags[q], &sown) != EI_IMPULSE_OK) {
            printf("call %s slide_create_%d -1\n", name, q);
            return;
        }
        printf("call %s slide_create_%d %d\n", name, q, kws_bank_slide_live_path(sessions[q]) == kws_slide_live_path(sown) ? 0 : -1);
        unsigned seed = 777 + q;
        size_t pushes = 0, mism = 0;
        std::vector<size_t> streams, offs, lens, nb, ns;
        Outputs w(b, 64);
        for (int it = 0; it < 60; it++) {
            streams.clear(); offs.clear(); lens.clear();
            for (size_t st = 0; st < S; st++) {
                if (rnd(seed) % 3 == 0) continue;
                const unsigned kind = rnd(seed) % 5;
                const size_t n = kind == 0 ? 0 : kind == 1 ? 1 : kind == 2 ? clip - 1 : kind == 3 ? hops[q] : rnd(seed) % 20000;
                streams.push_back(st); offs.push_back(1 + 2 * (rnd(seed) % 1000)); lens.push_back(n);
            }
            const size_t n = streams.size();
            nb.assign(n, 99); ns.assign(n, 98);
            for (size_t i = 0; i < n; i++) {
                size_t a = 0, c = 1;
                (void)kws_bank_slide_live_window_count(sessions[q], streams[i], lens[i], &a);
                (void)kws_slide_live_window_count(sown, streams[i], lens[i], &c);
                mism += a != c;
            }
            if (it == 30) { const size_t two[2] = { 1, 3 }; mism += kws_bank_slide_live_reset(sessions[q], two, 2) != EI_IMPULSE_OK || kws_slide_live_reset(sown, two, 2) != EI_IMPULSE_OK; }
            const EI_IMPULSE_ERROR rb = kws_bank_slide_live_push_device(sessions[q], n, streams.data(), pcm.data(), offs.data(), lens.data(), w.sp.data(), it & 1 ? w.feats.data() : nullptr, nb.data(), nullptr);
            const EI_IMPULSE_ERROR rs = kws_slide_live_push_device(sown, n, streams.data(), pcm.data(), offs.data(), lens.data(), w.sp[0], nullptr, ns.data(), nullptr);
            mism += rb != EI_IMPULSE_OK || rs != EI_IMPULSE_OK;
            for (size_t i = 0; i < n; i++) mism += nb[i] != ns[i];
            pushes++;
        }
        printf("counts %s slide_live_%d %zu %zu\n", name, q, pushes, mism);
        (void)kws_bank_slide_live_reset(sessions[q], nullptr, 0);
        (void)kws_slide_live_reset(sown, nullptr, 0);
        const size_t st2[2] = { 4, 1 }, of2[2] = { 5, 90001 }, ln2[2] = { clip + 3 * hops[q] + 7, clip };
        size_t nw[2];
        const std::string tag = "slide_push_" + std::to_string(q);
        { Section s(name, tag.c_str()); printf("call %s %s %d\n", name, tag.c_str(), (int)kws_bank_slide_live_push_device(sessions[q], 2, st2, pcm.data(), of2, ln2, w.sp.data(), w.feats.data(), nw, nullptr)); }
        { Section s(name, (tag + "_single").c_str()); printf("call %s %s_single %d\n", name, tag.c_str(), (int)kws_slide_live_push_device(sown, 2, st2, pcm.data(), of2, ln2, w.sp[0], w.feats.data(), nw, nullptr)); }
        kws_slide_live_destroy(sown);
    }
    {
        sl = sessions[0];
        const size_t st2[2] = { 0, 2 }, of2[2] = { 3, 70001 }, ln2[2] = { clip, clip + 17 }, tw[2] = { 2, 2 };
        size_t nw[2] = { 77, 77 }, before[2], after[2];
        auto mirrors = [&](size_t *out) { for (int i = 0; i < 2; i++) (void)kws_bank_slide_live_window_count(sl, st2[i], ln2[i], &out[i]); };
        mirrors(before);
        auto same = [&]() { mirrors(after); return after[0] == before[0] && after[1] == before[1] && nw[0] == 77 && nw[1] == 77 ? 1 : 0; };
        { Section s(name, "slide_push_nothing_wanted"); rc = kws_bank_slide_live_push_device(sl, 2, st2, pcm.data(), of2, ln2, o.none.data(), nullptr, nw, nullptr); refuse("slide_push_nothing_wanted", rc, same()); }
        { Section s(name, "slide_push_null_scores"); rc = kws_bank_slide_live_push_device(sl, 2, st2, pcm.data(), of2, ln2, nullptr, o.feats.data(), nw, nullptr); refuse("slide_push_null_scores", rc, same()); }
        { Section s(name, "slide_push_twice"); rc = kws_bank_slide_live_push_device(sl, 2, tw, pcm.data(), of2, ln2, o.sp.data(), nullptr, nw, nullptr); refuse("slide_push_twice", rc, same()); }
        { Section s(name, "slide_push_null_session"); rc = kws_bank_slide_live_push_device(nullptr, 2, st2, pcm.data(), of2, ln2, o.sp.data(), nullptr, nw, nullptr); refuse("slide_push_null_session", rc, same()); }
        { Section s(name, "slide_push_n0"); rc = kws_bank_slide_live_push_device(sl, 0, nullptr, nullptr, nullptr, nullptr, o.sp.data(), o.feats.data(), nullptr, nullptr); printf("empty %s slide_push_n0 %d %d\n", name, (int)rc, o.untouched() && same()); }
        const size_t few[2] = { clip - 1, 5 };
        { Section s(name, "slide_push_no_window"); rc = kws_bank_slide_live_push_device(sl, 2, st2, pcm.data(), of2, few, o.sp.data(), o.feats.data(), nw, nullptr); printf("nowindow %s slide_push_no_window %d %d\n", name, (int)rc, o.untouched() && nw[0] == 0 && nw[1] == 0); }
    }

    // ---- clips of their own lengths
    {
        const size_t B = 6;
        const size_t offs[6] = { 0, 16008, 32017, 48001, 64000, 90003 }, lens[6] = { clip, 640, clip - 1, 5000, clip + stride - 1, 12345 };
        const size_t zero_len[6] = { clip, 0, clip, clip, clip, clip }, too_long[6] = { clip, clip, clip, 2 * clip, clip, clip };
        { Section s(name, "ragged_null_bank"); refuse("ragged_null_bank", kws_bank_run_classifier_ragged_device(nullptr, pcm.data(), offs, lens, B, o.sp.data(), nullptr, nullptr)); }
        { Section s(name, "ragged_null_scores"); refuse("ragged_null_scores", kws_bank_run_classifier_ragged_device(b, pcm.data(), offs, lens, B, nullptr, o.feats.data(), nullptr)); }
        { Section s(name, "ragged_nothing_wanted"); refuse("ragged_nothing_wanted", kws_bank_run_classifier_ragged_device(b, pcm.data(), offs, lens, B, o.none.data(), nullptr, nullptr)); }
        { Section s(name, "ragged_no_frame"); refuse("ragged_no_frame", kws_bank_run_classifier_ragged_device(b, pcm.data(), offs, zero_len, B, o.sp.data(), o.feats.data(), nullptr)); }
        { Section s(name, "ragged_too_long"); refuse("ragged_too_long", kws_bank_run_classifier_ragged_device(b, pcm.data(), offs, too_long, B, o.sp.data(), o.feats.data(), nullptr)); }
        { Section s(name, "ragged_null_lengths"); refuse("ragged_null_lengths", kws_bank_run_classifier_ragged_device(b, pcm.data(), offs, nullptr, B, o.sp.data(), nullptr, nullptr)); }
        { Section s(name, "ragged_huge_batch"); refuse("ragged_huge_batch", kws_bank_run_classifier_ragged_device(b, pcm.data(), offs, lens, (size_t)1 << 31, o.sp.data(), nullptr, nullptr)); }
        { Section s(name, "ragged_b0"); rc = kws_bank_run_classifier_ragged_device(b, pcm.data(), nullptr, nullptr, 0, o.sp.data(), o.feats.data(), nullptr); printf("empty %s ragged_b0 %d %d\n", name, (int)rc, o.untouched()); }
        Outputs w(b, B);
        { Section s(name, "ragged"); printf("call %s ragged %d\n", name, (int)kws_bank_run_classifier_ragged_device(b, pcm.data(), offs, lens, B, w.sp.data(), w.feats.data(), nullptr)); }
        { Section s(name, "ragged_own_buffer"); printf("call %s ragged_own_buffer %d\n", name, (int)kws_bank_run_classifier_ragged_device(b, pcm.data(), offs, lens, B, w.sp.data(), nullptr, nullptr)); }
        { Section s(name, "ragged_features_only"); printf("call %s ragged_features_only %d\n", name, (int)kws_bank_run_classifier_ragged_device(b, pcm.data(), offs, lens, B, w.none.data(), w.feats.data(), nullptr)); }
        { Section s(name, "ragged_single"); printf("call %s ragged_single %d\n", name, (int)kws_run_classifier_ragged_device(h0, pcm.data(), offs, lens, B, w.sp[0], w.feats.data(), nullptr, nullptr)); }
    }
    // a member in fast mode: the calls neither follow nor change it
    {
        kws_handle *hl = kws_bank_member(b, K - 1);
        const bool fast = kws_set_mode(hl, KWS_MODE_FAST) == EI_IMPULSE_OK;
        Outputs w(b, 64);
        const size_t st1[1] = { 3 }, of1[1] = { 9 }, ln1[1] = { 5 * slice + 320 };
        size_t nw[1];
        (void)kws_bank_live_reset(lv, nullptr, 0);
        { Section s(name, "live_push_member_fast"); printf("call %s live_push_member_fast %d\n", name, (int)kws_bank_live_push_device(lv, 1, st1, pcm.data(), of1, ln1, nullptr, w.sp.data(), nullptr, nw, nullptr)); }
        printf("call %s mode_kept %d\n", name, kws_get_mode(hl) == (fast ? KWS_MODE_FAST : KWS_MODE_EXACT) ? 0 : -1);
        (void)kws_set_mode(hl, KWS_MODE_EXACT);
    }
    // sessions before their bank, in either order among themselves (even-sized banks: first created first; odd-sized: last created first)
    kws_live_destroy(own);
    if (K % 2 == 0) {
        kws_bank_live_destroy(lv);
        for (int q = 0; q < 3; q++) kws_bank_slide_live_destroy(sessions[q]);
    } else {
        for (int q = 2; q >= 0; q--) kws_bank_slide_live_destroy(sessions[q]);
        kws_bank_live_destroy(lv);
    }
    kws_bank_live_destroy(nullptr);
    kws_bank_slide_live_destroy(nullptr);
}

int main(int argc, char **argv)
{
    if (argc != 8) { fprintf(stderr, "usage: %s mfcc40 x 4, l476, l476_f32, l432\n", argv[0]); return 2; }
    kws_handle *h[7] = { nullptr };
    for (int i = 0; i < 7; i++) printf("load %d %d\n", i, (int)kws_create_from_file(argv[i + 1], 0, &h[i]));
    for (int i = 0; i < 7; i++) if (!h[i]) return 1;
    kws_handle *pair[2] = { h[4], h[5] }, *riap[2] = { h[5], h[4] };
    kws_bank *b40 = nullptr, *b13 = nullptr, *b13r = nullptr, *b1 = nullptr;
    if (kws_bank_create(h, 4, &b40) || kws_bank_create(pair, 2, &b13) || kws_bank_create(riap, 2, &b13r) || kws_bank_create(&h[6], 1, &b1)) return 1;
    exercise("mfcc40", b40);
    exercise("l476", b13);
    exercise("l476_reversed", b13r);
    exercise("l432_alone", b1);
    // banks over the same members in either order of destruction, all before their members
    kws_bank_destroy(b13r);
    kws_bank_destroy(b13);
    kws_bank_destroy(b1);
    kws_bank_destroy(b40);
    for (int i = 0; i < 7; i++) kws_destroy(h[i]);
    printf("done\n");
    return 0;
}
