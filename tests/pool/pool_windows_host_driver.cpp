// pool_windows_host_driver.cpp -- TEST INFRASTRUCTURE ONLY (tests/test_pool_windows_host.py): argument checks, the per-window member table
// and the host bookkeeping of the pool's window calls (kws_pool_scan_recordings_device, kws_pool_slide_recordings_device,
// kws_pool_cmvn_inference_device, kws_pool_slide_live_*) run against the stub HIP runtime of tests/sanitize (device memory = host heap,
// launches do nothing) under ASan + UBSan.  No value a kernel would write means anything here.  With KWS_STUB_RECORD set the stub records
// every launch; the driver brackets each call it wants counted with "BEGIN <pool> <name>" / "END" notes.
// usage: kws_pool_windows_san tenant40 x 6      prints
//   load <n> <code>
//   refuse <pool> <name> <code> <outputs and session state untouched: 1/0> <the first member's own call's code, or 1 where there is none> | <kws_last_error>
//   call <pool> <name> <code>                                                                    (recorded)
//   chunks <pool> <name> <gathered chunks of the call>
//   windows <pool> <name> <n_windows ...> | <kws_pool_slide_live_window_count before the push ...>
//   table <n> | <assign ...> | <index ..., or -> | <n_windows ...> | <the per-window members ...>
//   done
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../include/kws/kws.h"

extern "C" void kws_stub_note(const char *line);
// the library's per-window member table (csrc/kws_pool.h; internal, linked statically here)
void kws_pool_window_members(const uint32_t *assign, const size_t *index, const size_t *n_windows, size_t n, std::vector<uint32_t> &out);

static const float FILL = -7.0f;

static bool all_are(const std::vector<float> &v, float x)
{
    for (float f : v) if (f != x) return false;
    return true;
}

struct Section {
    Section(const char *pool, const char *name) { kws_stub_note((std::string("BEGIN ") + pool + " " + name).c_str()); }
    ~Section() { kws_stub_note("END"); }
};

struct Outputs {
    std::vector<float> sc, raw, feats;
    Outputs(kws_pool *p, size_t rows, size_t feature_rows)
        : sc(rows * kws_pool_score_stride(p), FILL), raw(rows * kws_pool_score_stride(p), FILL), feats(feature_rows * (size_t)kws_feature_count(kws_pool_member(p, 0)), FILL)
    {
    }
    int untouched() const { return all_are(sc, FILL) && all_are(raw, FILL) && all_are(feats, FILL) ? 1 : 0; }
};

static unsigned rnd(unsigned &s) { s = s * 1664525u + 1013904223u; return s >> 8; }

static void print_table(size_t n, size_t S, bool by_index, unsigned seed)
{
    unsigned s = seed;
    std::vector<uint32_t> assign(by_index ? S : n), out;
    std::vector<size_t> index(n), nw(n);
    for (uint32_t &a : assign) a = rnd(s) % 3 == 0 ? KWS_POOL_NONE : (uint32_t)(rnd(s) % 40);
    for (size_t i = 0; i < n; i++) { index[i] = rnd(s) % S; nw[i] = rnd(s) % 3 == 0 ? 0 : rnd(s) % 5; }
    kws_pool_window_members(assign.data(), by_index ? index.data() : nullptr, nw.data(), n, out);
    printf("table %zu |", n);
    for (uint32_t a : assign) printf(" %u", a);
    printf(" |");
    if (by_index) for (size_t i : index) printf(" %zu", i);
    else printf(" -");
    printf(" |");
    for (size_t w : nw) printf(" %zu", w);
    printf(" |");
    for (uint32_t m : out) printf(" %u", m);
    printf("\n");
}

static void exercise(const char *name, kws_pool *p)
{
    const size_t K = kws_pool_size(p);
    kws_handle *h0 = kws_pool_member(p, 0);
    const size_t clip = (size_t)kws_clip_samples(h0), F = (size_t)kws_feature_count(h0), slice = 4000, hop = 1600, S = 5;
    const size_t chunk = ((size_t)64 << 20) / (4 * F), big = chunk + 9;             // windows of one gathered chunk; a call of two chunks
    std::vector<int16_t> pcm(400000, 3);
    Outputs o(p, 64, 64);
    std::vector<float> own_sc(64 * (size_t)kws_label_count(h0), FILL), own_raw(own_sc);
    EI_IMPULSE_ERROR rc;
    auto refuse = [&](const char *what, EI_IMPULSE_ERROR code, int state_ok = 1, int own_code = 1) {
        printf("refuse %s %s %d %d %d | %s\n", name, what, (int)code, o.untouched() && state_ok, own_code, kws_last_error());
    };
    auto call = [&](const char *what, EI_IMPULSE_ERROR code) { printf("call %s %s %d\n", name, what, (int)code); };
    const uint32_t last = (uint32_t)(K - 1), second = (uint32_t)(1 % K);

    // six recordings: no samples, too short for a window (scan: 3 slices; slide: less than a clip), then 1, 3, 6 and 2 scan windows
    const size_t R = 6, offs[6] = { 3, 20001, 40001, 70001, 110001, 160001 }, lens[6] = { 0, 3 * slice + 5, 4 * slice, 6 * slice + 320, 9 * slice, 5 * slice };
    const uint32_t mixed[6] = { KWS_POOL_NONE, 0, last, KWS_POOL_NONE, 0, second }, none[6] = { KWS_POOL_NONE, KWS_POOL_NONE, KWS_POOL_NONE, KWS_POOL_NONE, KWS_POOL_NONE, KWS_POOL_NONE },
                   windowless[6] = { 0, last, KWS_POOL_NONE, KWS_POOL_NONE, KWS_POOL_NONE, KWS_POOL_NONE };
    uint32_t bad[6];
    memcpy(bad, mixed, sizeof(bad));
    bad[1] = (uint32_t)K;                        // (a recording without windows: its member is still checked) ...
    bad[4] = (uint32_t)K + 7u;                   // ... and it is the first that is named

    // ---- recording scans
    {
        { Section s(name, "scan_bad_index"); refuse("scan_bad_index", kws_pool_scan_recordings_device(p, pcm.data(), offs, lens, R, bad, slice, o.sc.data(), o.raw.data(), nullptr)); }
        { Section s(name, "scan_null_scores"); refuse("scan_null_scores", kws_pool_scan_recordings_device(p, pcm.data(), offs, lens, R, mixed, slice, nullptr, o.raw.data(), nullptr)); }
        { Section s(name, "scan_null_pool"); refuse("scan_null_pool", kws_pool_scan_recordings_device(nullptr, pcm.data(), offs, lens, R, mixed, slice, o.sc.data(), nullptr, nullptr)); }
        { Section s(name, "scan_null_member"); refuse("scan_null_member", kws_pool_scan_recordings_device(p, pcm.data(), offs, lens, R, nullptr, slice, o.sc.data(), nullptr, nullptr)); }
        {
            Section s(name, "scan_null_lengths");
            const int own = (int)kws_scan_recordings_device(h0, pcm.data(), offs, nullptr, R, slice, own_sc.data(), nullptr, nullptr);
            refuse("scan_null_lengths", kws_pool_scan_recordings_device(p, pcm.data(), offs, nullptr, R, mixed, slice, o.sc.data(), nullptr, nullptr), 1, own);
        }
        {
            Section s(name, "scan_bad_slicing");
            const int own = (int)kws_scan_recordings_device(h0, pcm.data(), offs, lens, R, 1234, own_sc.data(), nullptr, nullptr);
            refuse("scan_bad_slicing", kws_pool_scan_recordings_device(p, pcm.data(), offs, lens, R, mixed, 1234, o.sc.data(), nullptr, nullptr), all_are(own_sc, FILL), own);
        }
        Outputs w(p, 64, 1);
        { Section s(name, "own_scan"); call("own_scan", kws_scan_recordings_device(h0, pcm.data(), offs, lens, R, slice, own_sc.data(), own_raw.data(), nullptr)); }
        { Section s(name, "scan_mixed"); call("scan_mixed", kws_pool_scan_recordings_device(p, pcm.data(), offs, lens, R, mixed, slice, w.sc.data(), w.raw.data(), nullptr)); }
        { Section s(name, "scan_in_place"); call("scan_in_place", kws_pool_scan_recordings_device(p, pcm.data(), offs, lens, R, mixed, slice, w.sc.data(), nullptr, nullptr)); }
        { Section s(name, "scan_none"); call("scan_none", kws_pool_scan_recordings_device(p, pcm.data(), offs, lens, R, none, slice, w.sc.data(), w.raw.data(), nullptr)); }
        // members named only by recordings that have no window: neither pool kernel
        { Section s(name, "scan_windowless"); call("scan_windowless", kws_pool_scan_recordings_device(p, pcm.data(), offs, lens, R, windowless, slice, w.sc.data(), nullptr, nullptr)); }
        { Section s(name, "scan_r0"); call("scan_r0", kws_pool_scan_recordings_device(p, nullptr, nullptr, nullptr, 0, nullptr, slice, w.sc.data(), nullptr, nullptr)); }
    }

    // ---- slides over recordings
    {
        const size_t huge[1] = { (size_t)1 << 50 }, at0[1] = { 0 };
        { Section s(name, "slide_bad_index"); refuse("slide_bad_index", kws_pool_slide_recordings_device(p, pcm.data(), offs, lens, R, bad, hop, 0, o.sc.data(), o.feats.data(), nullptr)); }
        { Section s(name, "slide_no_output"); refuse("slide_no_output", kws_pool_slide_recordings_device(p, pcm.data(), offs, lens, R, mixed, hop, 0, nullptr, nullptr, nullptr)); }
        { Section s(name, "slide_null_pool"); refuse("slide_null_pool", kws_pool_slide_recordings_device(nullptr, pcm.data(), offs, lens, R, mixed, hop, 0, o.sc.data(), nullptr, nullptr)); }
        { Section s(name, "slide_null_member"); refuse("slide_null_member", kws_pool_slide_recordings_device(p, pcm.data(), offs, lens, R, nullptr, hop, 0, o.sc.data(), nullptr, nullptr)); }
        {
            Section s(name, "slide_null_lengths");
            const int own = (int)kws_slide_recordings_device(h0, pcm.data(), offs, nullptr, R, hop, 0, own_sc.data(), nullptr, nullptr);
            refuse("slide_null_lengths", kws_pool_slide_recordings_device(p, pcm.data(), offs, nullptr, R, mixed, hop, 0, o.sc.data(), nullptr, nullptr), 1, own);
        }
        {
            Section s(name, "slide_bad_hop");
            const int own = (int)kws_slide_recordings_device(h0, pcm.data(), offs, lens, R, 0, 0, own_sc.data(), nullptr, nullptr);
            refuse("slide_bad_hop", kws_pool_slide_recordings_device(p, pcm.data(), offs, lens, R, mixed, 0, 0, o.sc.data(), nullptr, nullptr), 1, own);
        }
        {
            Section s(name, "slide_bad_flags");
            const int own = (int)kws_slide_recordings_device(h0, pcm.data(), offs, lens, R, hop, 7, own_sc.data(), nullptr, nullptr);
            refuse("slide_bad_flags", kws_pool_slide_recordings_device(p, pcm.data(), offs, lens, R, mixed, hop, 7, o.sc.data(), nullptr, nullptr), 1, own);
        }
        {
            Section s(name, "slide_too_many_windows");
            const int own = (int)kws_slide_recordings_device(h0, pcm.data(), at0, huge, 1, 1, 0, own_sc.data(), nullptr, nullptr);
            refuse("slide_too_many_windows", kws_pool_slide_recordings_device(p, pcm.data(), at0, huge, 1, mixed + 1, 1, 0, o.sc.data(), nullptr, nullptr), all_are(own_sc, FILL), own);
        }
        Outputs w(p, 64, 64);
        { Section s(name, "own_slide"); call("own_slide", kws_slide_recordings_device(h0, pcm.data(), offs, lens, R, hop, 0, own_sc.data(), w.feats.data(), nullptr)); }
        { Section s(name, "slide_mixed"); call("slide_mixed", kws_pool_slide_recordings_device(p, pcm.data(), offs, lens, R, mixed, hop, 0, w.sc.data(), w.feats.data(), nullptr)); }
        { Section s(name, "slide_features_only"); call("slide_features_only", kws_pool_slide_recordings_device(p, pcm.data(), offs, lens, R, mixed, hop, 0, nullptr, w.feats.data(), nullptr)); }
        { Section s(name, "slide_none"); call("slide_none", kws_pool_slide_recordings_device(p, pcm.data(), offs, lens, R, none, hop, 0, w.sc.data(), nullptr, nullptr)); }
        // two gathered chunks: one recording of chunk + 9 windows one sample apart, and a short one of another member behind it
        const size_t o2[2] = { 1, 100001 }, l2[2] = { clip + big - 1, clip + 4 };
        const uint32_t m2[2] = { last, 0 };
        Outputs wide(p, big + 5, 1);
        std::vector<float> own_wide((big + 5) * (size_t)kws_label_count(h0), FILL);
        { Section s(name, "own_slide_two_chunks"); call("own_slide_two_chunks", kws_slide_recordings_device(h0, pcm.data(), o2, l2, 2, 1, 0, own_wide.data(), nullptr, nullptr)); }
        { Section s(name, "slide_two_chunks"); call("slide_two_chunks", kws_pool_slide_recordings_device(p, pcm.data(), o2, l2, 2, m2, 1, 0, wide.sc.data(), nullptr, nullptr)); }
        printf("chunks %s slide_two_chunks %zu\n", name, (big + 5 + chunk - 1) / chunk);
    }

    // ---- cepstra in
    {
        const size_t B = 9;
        std::vector<float> mfcc(B * F, 0.25f);
        std::vector<uint32_t> robin(B), nobody(B, KWS_POOL_NONE), wrong(B);
        for (size_t i = 0; i < B; i++) robin[i] = wrong[i] = (uint32_t)(i % K);
        wrong[3] = (uint32_t)K;
        wrong[5] = (uint32_t)K + 7u;
        { Section s(name, "cmvn_bad_index"); refuse("cmvn_bad_index", kws_pool_cmvn_inference_device(p, mfcc.data(), B, wrong.data(), o.sc.data(), o.feats.data(), nullptr)); }
        { Section s(name, "cmvn_no_output"); refuse("cmvn_no_output", kws_pool_cmvn_inference_device(p, mfcc.data(), B, robin.data(), nullptr, nullptr, nullptr)); }
        { Section s(name, "cmvn_null_pool"); refuse("cmvn_null_pool", kws_pool_cmvn_inference_device(nullptr, mfcc.data(), B, robin.data(), o.sc.data(), nullptr, nullptr)); }
        { Section s(name, "cmvn_null_member"); refuse("cmvn_null_member", kws_pool_cmvn_inference_device(p, mfcc.data(), B, nullptr, o.sc.data(), nullptr, nullptr)); }
        { Section s(name, "cmvn_null_mfcc"); refuse("cmvn_null_mfcc", kws_pool_cmvn_inference_device(p, nullptr, B, robin.data(), o.sc.data(), nullptr, nullptr)); }
        Outputs w(p, B, B);
        { Section s(name, "own_cmvn"); call("own_cmvn", kws_cmvn_inference_batch_device(h0, mfcc.data(), B, own_sc.data(), w.feats.data(), nullptr, nullptr)); }
        { Section s(name, "cmvn_robin"); call("cmvn_robin", kws_pool_cmvn_inference_device(p, mfcc.data(), B, robin.data(), w.sc.data(), w.feats.data(), nullptr)); }
        { Section s(name, "cmvn_no_features"); call("cmvn_no_features", kws_pool_cmvn_inference_device(p, mfcc.data(), B, robin.data(), w.sc.data(), nullptr, nullptr)); }
        { Section s(name, "cmvn_none"); call("cmvn_none", kws_pool_cmvn_inference_device(p, mfcc.data(), B, nobody.data(), w.sc.data(), w.feats.data(), nullptr)); }
        { Section s(name, "cmvn_features_only"); call("cmvn_features_only", kws_pool_cmvn_inference_device(p, mfcc.data(), B, robin.data(), nullptr, w.feats.data(), nullptr)); }
        { Section s(name, "cmvn_b0"); call("cmvn_b0", kws_pool_cmvn_inference_device(p, mfcc.data(), 0, nullptr, w.sc.data(), nullptr, nullptr)); }
    }

    // ---- live one-shot sessions
    {
        kws_pool_slide_live *none_yet = (kws_pool_slide_live *)(void *)&p;
        {
            Section s(name, "sl_create_bad_hop");
            kws_slide_live *own = nullptr;
            const int own_code = (int)kws_slide_live_create(h0, S, 0, 0, &own);
            rc = kws_pool_slide_live_create(p, S, 0, 0, &none_yet);
            refuse("sl_create_bad_hop", rc, none_yet == nullptr, own_code);
        }
        { Section s(name, "sl_create_null_pool"); rc = kws_pool_slide_live_create(nullptr, S, hop, 0, &none_yet); refuse("sl_create_null_pool", rc, none_yet == nullptr); }
        kws_slide_live *own = nullptr, *own_big = nullptr;
        kws_pool_slide_live *fresh = nullptr, *hot = nullptr, *wide_sl = nullptr;
        if (kws_slide_live_create(h0, S, hop, 0, &own) || kws_pool_slide_live_create(p, S, hop, 0, &fresh) || kws_pool_slide_live_create(p, S, hop, 0, &hot) ||
            kws_slide_live_create(h0, 2, 1, 0, &own_big) || kws_pool_slide_live_create(p, 2, 1, 0, &wide_sl)) { call("sl_create", (EI_IMPULSE_ERROR)-1); return; }
        printf("path %s %d %d\n", name, kws_pool_slide_live_path(hot), kws_slide_live_path(own));
        const size_t every_stream[5] = { 0, 1, 2, 3, 4 };
        uint32_t robin[5];
        for (size_t i = 0; i < S; i++) robin[i] = (uint32_t)(i % K);
        const size_t st3[3] = { 0, 1, 2 }, of3[3] = { 3, 70001, 140001 }, ln3[3] = { clip + 3 * hop + 5, clip + 2 * hop, clip - 1 };
        size_t nw[3] = { 0, 0, 0 }, cnt[3] = { 9, 9, 9 };
        Outputs w(p, 64, 64);
        { Section s(name, "own_sl_push"); call("own_sl_push", kws_slide_live_push_device(own, 3, st3, pcm.data(), of3, ln3, own_sc.data(), w.feats.data(), nw, nullptr)); }
        // a fresh session assigns every stream to nobody: the windows are counted, the features written, no network runs
        for (size_t i = 0; i < 3; i++) (void)kws_pool_slide_live_window_count(fresh, st3[i], ln3[i], &cnt[i]);
        { Section s(name, "sl_push_unassigned"); call("sl_push_unassigned", kws_pool_slide_live_push_device(fresh, 3, st3, pcm.data(), of3, ln3, w.sc.data(), w.feats.data(), nw, nullptr)); }
        printf("windows %s sl_push_unassigned %zu %zu %zu | %zu %zu %zu\n", name, nw[0], nw[1], nw[2], cnt[0], cnt[1], cnt[2]);
        { Section s(name, "sl_assign"); call("sl_assign", kws_pool_slide_live_assign(hot, every_stream, S, robin)); }
        for (size_t i = 0; i < 3; i++) (void)kws_pool_slide_live_window_count(hot, st3[i], ln3[i], &cnt[i]);
        { Section s(name, "sl_push_assigned"); call("sl_push_assigned", kws_pool_slide_live_push_device(hot, 3, st3, pcm.data(), of3, ln3, w.sc.data(), nullptr, nw, nullptr)); }
        printf("windows %s sl_push_assigned %zu %zu %zu | %zu %zu %zu\n", name, nw[0], nw[1], nw[2], cnt[0], cnt[1], cnt[2]);
        // refusals: nothing changes
        const size_t s44[2] = { 4, 4 }, far[1] = { S }, one4[1] = { 4 }, of1[1] = { 9 }, ln1[1] = { clip + hop }, s33[2] = { 3, 3 }, of2[2] = { 9, 50001 }, ln2[2] = { hop, hop };
        const uint32_t other[2] = { second, KWS_POOL_NONE }, badidx[1] = { (uint32_t)K }, none1[1] = { KWS_POOL_NONE };
        size_t before = 0, after = 0, n1[2] = { 77, 77 };
        (void)kws_pool_slide_live_window_count(hot, 0, hop, &before);
        auto same = [&]() { (void)kws_pool_slide_live_window_count(hot, 0, hop, &after); return after == before ? 1 : 0; };
        { Section s(name, "sl_assign_range"); rc = kws_pool_slide_live_assign(hot, far, 1, none1); refuse("sl_assign_range", rc, same()); }
        { Section s(name, "sl_assign_twice"); rc = kws_pool_slide_live_assign(hot, s44, 2, other); refuse("sl_assign_twice", rc, same()); }
        { Section s(name, "sl_assign_bad_index"); rc = kws_pool_slide_live_assign(hot, one4, 1, badidx); refuse("sl_assign_bad_index", rc, same()); }
        { Section s(name, "sl_assign_null_session"); rc = kws_pool_slide_live_assign(nullptr, one4, 1, none1); refuse("sl_assign_null_session", rc, same()); }
        { Section s(name, "sl_assign_null_member"); rc = kws_pool_slide_live_assign(hot, one4, 1, nullptr); refuse("sl_assign_null_member", rc, same()); }
        { Section s(name, "sl_push_stream_range"); rc = kws_pool_slide_live_push_device(hot, 1, far, pcm.data(), of1, ln1, o.sc.data(), nullptr, n1, nullptr); refuse("sl_push_stream_range", rc, same() && n1[0] == 77); }
        { Section s(name, "sl_push_stream_twice"); rc = kws_pool_slide_live_push_device(hot, 2, s33, pcm.data(), of2, ln2, o.sc.data(), nullptr, n1, nullptr); refuse("sl_push_stream_twice", rc, same() && n1[0] == 77); }
        { Section s(name, "sl_push_no_output"); rc = kws_pool_slide_live_push_device(hot, 1, one4, pcm.data(), of1, ln1, nullptr, nullptr, n1, nullptr); refuse("sl_push_no_output", rc, same() && n1[0] == 77); }
        { Section s(name, "sl_push_null_session"); rc = kws_pool_slide_live_push_device(nullptr, 1, one4, pcm.data(), of1, ln1, o.sc.data(), nullptr, n1, nullptr); refuse("sl_push_null_session", rc, same()); }
        // a member may change between any two pushes: stream 0 has been pushed to and is unassigned, then pushed again (no network), then
        // given another member and pushed once more
        { Section s(name, "sl_unassign_after_push"); call("sl_unassign_after_push", kws_pool_slide_live_assign(hot, st3, 1, none1)); }
        const size_t of0[1] = { 5 }, ln0[1] = { 2 * hop };
        { Section s(name, "sl_push_after_unassign"); call("sl_push_after_unassign", kws_pool_slide_live_push_device(hot, 1, st3, pcm.data(), of0, ln0, w.sc.data(), nullptr, n1, nullptr)); }
        { Section s(name, "sl_assign_after_push"); call("sl_assign_after_push", kws_pool_slide_live_assign(hot, st3, 1, other)); }
        { Section s(name, "sl_push_reassigned"); call("sl_push_reassigned", kws_pool_slide_live_push_device(hot, 1, st3, pcm.data(), of0, ln0, w.sc.data(), nullptr, n1, nullptr)); }
        printf("windows %s sl_push_reassigned %zu | 2\n", name, n1[0]);
        // a reset keeps members: stream 1's first clip gives one window and one network launch
        call("sl_reset", kws_pool_slide_live_reset(hot, st3 + 1, 1));
        const size_t ofc[1] = { 7 }, lnc[1] = { clip };
        { Section s(name, "sl_push_after_reset"); call("sl_push_after_reset", kws_pool_slide_live_push_device(hot, 1, st3 + 1, pcm.data(), ofc, lnc, w.sc.data(), nullptr, n1, nullptr)); }
        printf("windows %s sl_push_after_reset %zu | 1\n", name, n1[0]);
        { Section s(name, "sl_push_empty"); call("sl_push_empty", kws_pool_slide_live_push_device(hot, 0, nullptr, nullptr, nullptr, nullptr, w.sc.data(), nullptr, n1, nullptr)); }
        // two gathered chunks in one push: chunk + 9 windows one sample apart on stream 0, five more on stream 1
        const size_t st2[2] = { 0, 1 }, o2[2] = { 1, 100001 }, l2[2] = { clip + big - 1, clip + 4 };
        const uint32_t m2[2] = { last, 0 };
        size_t nw2[2] = { 0, 0 };
        Outputs wide(p, big + 5, 1);
        std::vector<float> own_wide((big + 5) * (size_t)kws_label_count(h0), FILL);
        call("sl_assign_two_chunks", kws_pool_slide_live_assign(wide_sl, st2, 2, m2));
        { Section s(name, "own_sl_push_two_chunks"); call("own_sl_push_two_chunks", kws_slide_live_push_device(own_big, 2, st2, pcm.data(), o2, l2, own_wide.data(), nullptr, nw2, nullptr)); }
        { Section s(name, "sl_push_two_chunks"); call("sl_push_two_chunks", kws_pool_slide_live_push_device(wide_sl, 2, st2, pcm.data(), o2, l2, wide.sc.data(), nullptr, nw2, nullptr)); }
        printf("chunks %s sl_push_two_chunks %zu\n", name, (nw2[0] + nw2[1] + chunk - 1) / chunk);
        kws_pool_slide_live_destroy(wide_sl);
        kws_pool_slide_live_destroy(hot);
        kws_pool_slide_live_destroy(fresh);
        kws_pool_slide_live_destroy(nullptr);
        kws_slide_live_destroy(own_big);
        kws_slide_live_destroy(own);
    }
}

int main(int argc, char **argv)
{
    if (argc != 7) { fprintf(stderr, "usage: %s tenant40 x 6\n", argv[0]); return 2; }
    kws_handle *h[6] = { nullptr };
    for (int i = 0; i < 6; i++) printf("load %d %d\n", i, (int)kws_create_from_file(argv[i + 1], 0, &h[i]));
    for (int i = 0; i < 6; i++) if (!h[i]) return 1;
    kws_pool *p6 = nullptr, *p1 = nullptr;
    if (kws_pool_create(h, 6, &p6) || kws_pool_create(&h[2], 1, &p1)) { fprintf(stderr, "%s\n", kws_last_error()); return 1; }
    printf("pool six %zu %zu\n", kws_pool_size(p6), kws_pool_score_stride(p6));
    exercise("six", p6);
    exercise("alone", p1);
    // the per-window member table as host arithmetic: by recording (index == NULL) and by stream
    unsigned seed = 7;
    for (size_t n : { (size_t)0, (size_t)1, (size_t)9, (size_t)40 }) {
        print_table(n, 12, false, seed++);
        print_table(n, 12, true, seed++);
    }
    kws_pool_destroy(p1);
    kws_pool_destroy(p6);
    for (int i = 0; i < 6; i++) kws_destroy(h[i]);
    printf("done\n");
    return 0;
}
