// bank_route_recordings_host_driver.cpp -- TEST INFRASTRUCTURE ONLY (tests/test_bank_route_recordings_host.py): argument checks, the
// per-window route table and the host bookkeeping of the routed recording and cepstra-in calls (kws_bank_scan_recordings_routed_device,
// kws_bank_slide_recordings_routed_device, kws_bank_cmvn_inference_routed_device) run against the stub HIP runtime of tests/sanitize (device
// memory = host heap, launches do nothing) under ASan + UBSan.  No value a kernel would write means anything here.  With KWS_STUB_RECORD set
// the stub records every launch; the driver brackets each call it wants counted with "BEGIN <bank> <name>" / "END" notes.
// usage: kws_bank_route_recordings_san mfcc40_a mfcc40_b mfcc40_c mfcc40_d l476 l476_f32 l432      prints
//   load <n> <code>
//   refuse <bank> <name> <code> <outputs untouched: 1/0> | <kws_last_error>                      (recorded: must launch nothing)
//   call <bank> <name> <code>                                                                    (recorded)
//   labels <bank> | <label count of every member>
//   windows <bank> <scan|slide> | <window count of every recording of the bank's section>
//   table <n> | <routes ...> | <index ... or -> | <window counts ...> | <the per-window table ...>
//   done
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../include/kws/kws.h"

extern "C" void kws_stub_note(const char *line);
// the library's table builder (csrc/kws_bank.h; internal, linked statically here)
void kws_bank_window_routes(const uint32_t *route, const size_t *index, const size_t *n_windows, size_t n, std::vector<uint32_t> &out);

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
    std::vector<float *> sp, rp;
    std::vector<float> feats;
    Outputs(kws_bank *b, size_t rows)
    {
        const size_t K = kws_bank_size(b);
        sc.resize(K); raw.resize(K); sp.resize(K); rp.resize(K);
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

static void print_table(const std::vector<uint32_t> &route, const std::vector<size_t> *index, const std::vector<size_t> &nw)
{
    std::vector<uint32_t> out(3, 77u);                  // (stale contents must go)
    kws_bank_window_routes(route.data(), index ? index->data() : nullptr, nw.data(), nw.size(), out);
    printf("table %zu |", nw.size());
    for (uint32_t r : route) printf(" %u", r);
    printf(" |");
    if (index) for (size_t i : *index) printf(" %zu", i);
    else printf(" -");
    printf(" |");
    for (size_t w : nw) printf(" %zu", w);
    printf(" |");
    for (uint32_t r : out) printf(" %u", r);
    printf("\n");
}

static void exercise(const char *name, kws_bank *b)
{
    const size_t K = kws_bank_size(b);
    const uint32_t every = (1u << K) - 1u, last = 1u << (K - 1);
    kws_handle *h0 = kws_bank_member(b, 0);
    const size_t clip = (size_t)kws_clip_samples(h0), stride = (size_t)kws_frame_stride_samples(h0), slice = 4000;
    std::vector<int16_t> pcm(400000, 3);
    printf("labels %s |", name);
    for (size_t k = 0; k < K; k++) printf(" %d", kws_label_count(kws_bank_member(b, k)));
    printf("\n");
    Outputs o(b, 256);
    std::vector<float *> no_buffers(K, nullptr);
    auto refuse = [&](const char *what, EI_IMPULSE_ERROR code) { printf("refuse %s %s %d %d | %s\n", name, what, (int)code, o.untouched(), kws_last_error()); };
    auto call = [&](const char *what, EI_IMPULSE_ERROR code) { printf("call %s %s %d\n", name, what, (int)code); };
#define REFUSE(what, expr) do { Section s_(name, what); refuse(what, expr); } while (0)
#define CALL(what, expr) do { Section s_(name, what); call(what, expr); } while (0)

    // ---- recording scans: recordings 1 and 4 are too short for a window (1 between two recordings that have windows, none at the very end
    //      here: the table lines below put them at the front and the end too)
    {
        const size_t R = 6;
        const size_t offs[6] = { 3, 30001, 50001, 80001, 110001, 120001 };
        const size_t lens[6] = { 7 * slice + 320, 2 * slice, 6 * slice + 320, 5 * slice + 320, slice, 9 * slice + 7 };
        printf("windows %s scan |", name);
        for (size_t r = 0; r < R; r++) { size_t w = 99; (void)kws_scan_window_count(h0, lens[r], slice, &w); printf(" %zu", w); }
        printf("\n");
        uint32_t all[6], all_but_short[6], onehot[6], first[6], lastm[6], none[6], bad[6], short_names[6];
        for (size_t r = 0; r < R; r++) {
            all[r] = all_but_short[r] = bad[r] = every; onehot[r] = 1u << (r % K); first[r] = 1u; lastm[r] = last; none[r] = 0u; short_names[r] = 1u;
        }
        all_but_short[1] = 0u; all_but_short[4] = 1u;            // (recordings without a window: their routes name no row)
        short_names[1] = short_names[4] = last;                  // only zero-window recordings name the last member
        bad[2] = every | (1u << K);
        bad[4] = 1u << 20;
        const uint32_t far[1] = { 1u << 30 };
        const size_t short_len[2] = { slice, 2 * slice };
        const uint32_t short_bad[2] = { 1u, (uint32_t)(1u << K) };
        REFUSE("scan_routed_bad_bit", kws_bank_scan_recordings_routed_device(b, pcm.data(), offs, lens, R, bad, slice, o.sp.data(), o.rp.data(), nullptr));
        REFUSE("scan_routed_null_bank", kws_bank_scan_recordings_routed_device(nullptr, pcm.data(), offs, lens, R, onehot, slice, o.sp.data(), nullptr, nullptr));
        REFUSE("scan_routed_null_pcm", kws_bank_scan_recordings_routed_device(b, nullptr, offs, lens, R, onehot, slice, o.sp.data(), nullptr, nullptr));
        REFUSE("scan_routed_null_scores", kws_bank_scan_recordings_routed_device(b, pcm.data(), offs, lens, R, onehot, slice, nullptr, nullptr, nullptr));
        REFUSE("scan_routed_nothing_wanted", kws_bank_scan_recordings_routed_device(b, pcm.data(), offs, lens, R, onehot, slice, no_buffers.data(), nullptr, nullptr));
        REFUSE("scan_routed_bad_slicing", kws_bank_scan_recordings_routed_device(b, pcm.data(), offs, lens, R, onehot, 7, o.sp.data(), nullptr, nullptr));
        REFUSE("scan_routed_short_bad_bit", kws_bank_scan_recordings_routed_device(b, pcm.data(), offs, short_len, 2, short_bad, slice, o.sp.data(), nullptr, nullptr));
        REFUSE("scan_null_routes_null_pcm", kws_bank_scan_recordings_routed_device(b, nullptr, offs, lens, R, nullptr, slice, o.sp.data(), nullptr, nullptr));
        REFUSE("scan_null_routes_bad_slicing", kws_bank_scan_recordings_routed_device(b, pcm.data(), offs, lens, R, nullptr, 7, o.sp.data(), nullptr, nullptr));
        REFUSE("scan_null_routes_nothing_wanted", kws_bank_scan_recordings_routed_device(b, pcm.data(), offs, lens, R, nullptr, slice, no_buffers.data(), nullptr, nullptr));
        Outputs w(b, 64);
        CALL("scan_unrouted", kws_bank_scan_recordings_device(b, pcm.data(), offs, lens, R, slice, w.sp.data(), w.rp.data(), nullptr));
        CALL("scan_null_routes", kws_bank_scan_recordings_routed_device(b, pcm.data(), offs, lens, R, nullptr, slice, w.sp.data(), w.rp.data(), nullptr));
        CALL("scan_all_routes", kws_bank_scan_recordings_routed_device(b, pcm.data(), offs, lens, R, all, slice, w.sp.data(), w.rp.data(), nullptr));
        CALL("scan_all_but_short", kws_bank_scan_recordings_routed_device(b, pcm.data(), offs, lens, R, all_but_short, slice, w.sp.data(), w.rp.data(), nullptr));
        CALL("scan_onehot", kws_bank_scan_recordings_routed_device(b, pcm.data(), offs, lens, R, onehot, slice, w.sp.data(), w.rp.data(), nullptr));
        CALL("scan_onehot_in_place", kws_bank_scan_recordings_routed_device(b, pcm.data(), offs, lens, R, onehot, slice, w.sp.data(), nullptr, nullptr));
        CALL("scan_first_only", kws_bank_scan_recordings_routed_device(b, pcm.data(), offs, lens, R, first, slice, w.sp.data(), nullptr, nullptr));
        CALL("scan_last_only", kws_bank_scan_recordings_routed_device(b, pcm.data(), offs, lens, R, lastm, slice, w.sp.data(), nullptr, nullptr));
        CALL("scan_none", kws_bank_scan_recordings_routed_device(b, pcm.data(), offs, lens, R, none, slice, w.sp.data(), w.rp.data(), nullptr));
        CALL("scan_short_names_last", kws_bank_scan_recordings_routed_device(b, pcm.data(), offs, lens, R, short_names, slice, w.sp.data(), w.rp.data(), nullptr));
        {
            // the first member is routed but has no buffer: skipped, as in the unrouted scan
            std::vector<float *> without(w.sp);
            without[0] = nullptr;
            CALL("scan_first_only_no_buffer", kws_bank_scan_recordings_routed_device(b, pcm.data(), offs, lens, R, first, slice, K > 1 ? without.data() : w.sp.data(), nullptr, nullptr));
        }
        // R = 0: no route is read (the batch routed call's rule: the routes [R] are checked, then the empty call returns)
        CALL("scan_r0", kws_bank_scan_recordings_routed_device(b, pcm.data(), offs, lens, 0, far, slice, w.sp.data(), nullptr, nullptr));
        CALL("scan_short", kws_bank_scan_recordings_routed_device(b, pcm.data(), offs, short_len, 2, first, slice, w.sp.data(), nullptr, nullptr));
    }

    // ---- slides: recordings 1 and 4 are shorter than a clip
    {
        const size_t R = 5, hop = 5 * stride;
        const size_t offs[5] = { 5, 60001, 90001, 130001, 170001 };
        const size_t lens[5] = { clip + 3 * hop + 7, clip - 1, clip, clip + hop, 100 };
        printf("windows %s slide |", name);
        for (size_t r = 0; r < R; r++) { size_t w = 99; (void)kws_slide_window_count(h0, lens[r], hop, &w); printf(" %zu", w); }
        printf("\n");
        uint32_t all[5], all_but_short[5], onehot[5], none[5], bad[5], short_names[5];
        for (size_t r = 0; r < R; r++) { all[r] = all_but_short[r] = bad[r] = every; onehot[r] = 1u << (r % K); none[r] = 0u; short_names[r] = 1u; }
        all_but_short[1] = 0u; all_but_short[4] = 1u;
        short_names[1] = short_names[4] = last;
        bad[3] = 1u << K;
        const uint32_t far[1] = { 1u << 30 };
        const size_t short_len[2] = { clip - 1, 7 };
        const uint32_t short_bad[2] = { 1u, (uint32_t)(1u << K) }, short_ok[2] = { 1u, 0u };
        REFUSE("slide_routed_bad_bit", kws_bank_slide_recordings_routed_device(b, pcm.data(), offs, lens, R, bad, hop, 0, o.sp.data(), o.feats.data(), nullptr));
        REFUSE("slide_routed_null_bank", kws_bank_slide_recordings_routed_device(nullptr, pcm.data(), offs, lens, R, onehot, hop, 0, o.sp.data(), nullptr, nullptr));
        REFUSE("slide_routed_null_pcm", kws_bank_slide_recordings_routed_device(b, nullptr, offs, lens, R, onehot, hop, 0, o.sp.data(), nullptr, nullptr));
        REFUSE("slide_routed_null_scores", kws_bank_slide_recordings_routed_device(b, pcm.data(), offs, lens, R, onehot, hop, 0, nullptr, o.feats.data(), nullptr));
        REFUSE("slide_routed_nothing_wanted", kws_bank_slide_recordings_routed_device(b, pcm.data(), offs, lens, R, onehot, hop, 0, no_buffers.data(), nullptr, nullptr));
        REFUSE("slide_routed_bad_hop", kws_bank_slide_recordings_routed_device(b, pcm.data(), offs, lens, R, onehot, 0, 0, o.sp.data(), nullptr, nullptr));
        REFUSE("slide_routed_bad_flags", kws_bank_slide_recordings_routed_device(b, pcm.data(), offs, lens, R, onehot, hop, 77, o.sp.data(), nullptr, nullptr));
        REFUSE("slide_routed_short_bad_bit", kws_bank_slide_recordings_routed_device(b, pcm.data(), offs, short_len, 2, short_bad, hop, 0, o.sp.data(), nullptr, nullptr));
        REFUSE("slide_null_routes_null_pcm", kws_bank_slide_recordings_routed_device(b, nullptr, offs, lens, R, nullptr, hop, 0, o.sp.data(), nullptr, nullptr));
        REFUSE("slide_null_routes_bad_hop", kws_bank_slide_recordings_routed_device(b, pcm.data(), offs, lens, R, nullptr, 0, 0, o.sp.data(), nullptr, nullptr));
        REFUSE("slide_null_routes_bad_flags", kws_bank_slide_recordings_routed_device(b, pcm.data(), offs, lens, R, nullptr, hop, 77, o.sp.data(), nullptr, nullptr));
        Outputs w(b, 16);
        for (int flags = 0; flags < 3; flags++) {               // KWS_SLIDE_AUTO, _DIRECT, _SHARED
            const std::string f = flags == 0 ? "" : flags == KWS_SLIDE_DIRECT ? "_direct" : "_shared";
            CALL(("slide_unrouted" + f).c_str(), kws_bank_slide_recordings_device(b, pcm.data(), offs, lens, R, hop, flags, w.sp.data(), w.feats.data(), nullptr));
            CALL(("slide_null_routes" + f).c_str(), kws_bank_slide_recordings_routed_device(b, pcm.data(), offs, lens, R, nullptr, hop, flags, w.sp.data(), w.feats.data(), nullptr));
            CALL(("slide_all_routes" + f).c_str(), kws_bank_slide_recordings_routed_device(b, pcm.data(), offs, lens, R, all, hop, flags, w.sp.data(), w.feats.data(), nullptr));
            CALL(("slide_onehot" + f).c_str(), kws_bank_slide_recordings_routed_device(b, pcm.data(), offs, lens, R, onehot, hop, flags, w.sp.data(), w.feats.data(), nullptr));
        }
        CALL("slide_all_but_short", kws_bank_slide_recordings_routed_device(b, pcm.data(), offs, lens, R, all_but_short, hop, 0, w.sp.data(), w.feats.data(), nullptr));
        CALL("slide_none", kws_bank_slide_recordings_routed_device(b, pcm.data(), offs, lens, R, none, hop, 0, w.sp.data(), w.feats.data(), nullptr));
        CALL("slide_short_names_last", kws_bank_slide_recordings_routed_device(b, pcm.data(), offs, lens, R, short_names, hop, 0, w.sp.data(), nullptr, nullptr));
        CALL("slide_r0", kws_bank_slide_recordings_routed_device(b, pcm.data(), offs, lens, 0, far, hop, 0, w.sp.data(), nullptr, nullptr));
        CALL("slide_short", kws_bank_slide_recordings_routed_device(b, pcm.data(), offs, short_len, 2, short_ok, hop, 0, w.sp.data(), nullptr, nullptr));
    }

    // ---- cepstra in
    {
        const size_t B = 9, F = (size_t)kws_feature_count(h0);
        std::vector<float> mfcc(B * F, 0.25f);
        std::vector<uint32_t> all(B, every), onehot(B), first(B, 1u), lastm(B, last), none(B, 0u), bad(B, every);
        for (size_t i = 0; i < B; i++) onehot[i] = 1u << (i % K);
        bad[3] = every | (1u << K);
        bad[5] = 1u << 20;
        const uint32_t far[1] = { 1u << 30 };
        REFUSE("cmvn_routed_bad_bit", kws_bank_cmvn_inference_routed_device(b, mfcc.data(), B, bad.data(), o.sp.data(), o.feats.data(), nullptr));
        REFUSE("cmvn_routed_null_bank", kws_bank_cmvn_inference_routed_device(nullptr, mfcc.data(), B, onehot.data(), o.sp.data(), nullptr, nullptr));
        REFUSE("cmvn_routed_null_mfcc", kws_bank_cmvn_inference_routed_device(b, nullptr, B, onehot.data(), o.sp.data(), nullptr, nullptr));
        REFUSE("cmvn_routed_null_scores", kws_bank_cmvn_inference_routed_device(b, mfcc.data(), B, onehot.data(), nullptr, o.feats.data(), nullptr));
        REFUSE("cmvn_routed_nothing_wanted", kws_bank_cmvn_inference_routed_device(b, mfcc.data(), B, onehot.data(), no_buffers.data(), nullptr, nullptr));
        REFUSE("cmvn_null_routes_null_mfcc", kws_bank_cmvn_inference_routed_device(b, nullptr, B, nullptr, o.sp.data(), nullptr, nullptr));
        REFUSE("cmvn_null_routes_nothing_wanted", kws_bank_cmvn_inference_routed_device(b, mfcc.data(), B, nullptr, no_buffers.data(), nullptr, nullptr));
        Outputs w(b, B);
        CALL("cmvn_unrouted", kws_bank_cmvn_inference_batch_device(b, mfcc.data(), B, w.sp.data(), w.feats.data(), nullptr));
        CALL("cmvn_null_routes", kws_bank_cmvn_inference_routed_device(b, mfcc.data(), B, nullptr, w.sp.data(), w.feats.data(), nullptr));
        CALL("cmvn_all_routes", kws_bank_cmvn_inference_routed_device(b, mfcc.data(), B, all.data(), w.sp.data(), w.feats.data(), nullptr));
        CALL("cmvn_onehot", kws_bank_cmvn_inference_routed_device(b, mfcc.data(), B, onehot.data(), w.sp.data(), w.feats.data(), nullptr));
        CALL("cmvn_first_only", kws_bank_cmvn_inference_routed_device(b, mfcc.data(), B, first.data(), w.sp.data(), nullptr, nullptr));
        CALL("cmvn_last_only", kws_bank_cmvn_inference_routed_device(b, mfcc.data(), B, lastm.data(), w.sp.data(), nullptr, nullptr));
        CALL("cmvn_none", kws_bank_cmvn_inference_routed_device(b, mfcc.data(), B, none.data(), w.sp.data(), w.feats.data(), nullptr));
        CALL("cmvn_b0", kws_bank_cmvn_inference_routed_device(b, mfcc.data(), 0, far, w.sp.data(), w.feats.data(), nullptr));
    }
#undef REFUSE
#undef CALL
}

int main(int argc, char **argv)
{
    if (argc != 8) { fprintf(stderr, "usage: %s mfcc40 x 4, l476, l476_f32, l432\n", argv[0]); return 2; }
    kws_handle *h[7] = { nullptr };
    for (int i = 0; i < 7; i++) printf("load %d %d\n", i, (int)kws_create_from_file(argv[i + 1], 0, &h[i]));
    for (int i = 0; i < 7; i++) if (!h[i]) return 1;
    kws_handle *pair[2] = { h[4], h[5] };
    kws_bank *b40 = nullptr, *b13 = nullptr, *b1 = nullptr;
    if (kws_bank_create(h, 4, &b40) || kws_bank_create(pair, 2, &b13) || kws_bank_create(&h[6], 1, &b1)) return 1;
    exercise("mfcc40", b40);
    exercise("l476", b13);
    exercise("l432_alone", b1);
    // the per-window table as host arithmetic, from (routes per recording, window counts): the counts are the scan's own for recordings of
    // 0 .. 11 slices, so recordings without a window sit at the front, in the middle and at the end; then the live form (routes by stream)
    {
        const size_t slice = 4000, slices[] = { 2, 0, 7, 4, 3, 11, 1, 5, 3 };
        std::vector<size_t> nw;
        std::vector<uint32_t> route;
        for (size_t i = 0; i < sizeof slices / sizeof slices[0]; i++) {
            size_t w = 0;
            if (kws_scan_window_count(h[4], slices[i] * slice + 123, slice, &w)) return 1;
            nw.push_back(w);
            route.push_back((uint32_t)(i * 5u + 1u) & 15u);
        }
        print_table(route, nullptr, nw);
        print_table(route, nullptr, std::vector<size_t>(route.size(), 0));             // no window at all
        print_table({ 9u }, nullptr, { 6 });
        print_table({}, nullptr, {});
        const std::vector<size_t> streams = { 4, 0, 2 };
        print_table({ 1u, 2u, 4u, 8u, 3u }, &streams, { 2, 0, 3 });
    }
    kws_bank_destroy(b13);
    kws_bank_destroy(b1);
    kws_bank_destroy(b40);
    for (int i = 0; i < 7; i++) kws_destroy(h[i]);
    printf("done\n");
    return 0;
}
