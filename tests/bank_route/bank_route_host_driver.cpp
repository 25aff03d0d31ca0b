// bank_route_host_driver.cpp -- TEST INFRASTRUCTURE ONLY (tests/test_bank_route_host.py): argument checks, list building and the host
// bookkeeping of the routed bank calls (kws_bank_run_classifier_routed_device, kws_bank_run_classifier_ragged_routed_device,
// kws_bank_live_route, kws_bank_slide_live_route) run against the stub HIP runtime of tests/sanitize (device memory = host heap, launches do
// nothing) under ASan + UBSan.  No value a kernel would write means anything here.  With KWS_STUB_RECORD set the stub records every launch;
// the driver brackets each call it wants counted with "BEGIN <bank> <name>" / "END" notes.
// usage: kws_bank_route_san mfcc40_a mfcc40_b mfcc40_c mfcc40_d l476 l476_f32 l432      prints
//   load <n> <code>
//   refuse <bank> <name> <code> <outputs and session state untouched: 1/0> | <kws_last_error>     (recorded: must launch nothing)
//   call <bank> <name> <code>                                                                    (recorded)
//   lists <K> <n> <seed> | <routes ...> | <the packed lists ...> | <at[0 .. K]>
//   done
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../include/kws/kws.h"

extern "C" void kws_stub_note(const char *line);
// the library's list builder (csrc/kws_bank.h; internal, linked statically here)
void kws_bank_route_lists(const uint32_t *routes, size_t n, size_t K, std::vector<int> &out, size_t *at);

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

static unsigned rnd(unsigned &s) { s = s * 1664525u + 1013904223u; return s >> 8; }

static void print_lists(size_t K, size_t n, unsigned seed)
{
    std::vector<uint32_t> routes(n);
    unsigned s = seed;
    for (size_t i = 0; i < n; i++) routes[i] = rnd(s) % 4 == 0 ? 0u : (uint32_t)(rnd(s) & ((1u << K) - 1u));
    std::vector<int> out;
    size_t at[17];
    kws_bank_route_lists(routes.data(), n, K, out, at);
    printf("lists %zu %zu %u |", K, n, seed);
    for (uint32_t r : routes) printf(" %u", r);
    printf(" |");
    for (int v : out) printf(" %d", v);
    printf(" |");
    for (size_t k = 0; k <= K; k++) printf(" %zu", at[k]);
    printf("\n");
}

static void exercise(const char *name, kws_bank *b)
{
    const size_t K = kws_bank_size(b);
    const uint32_t every = (1u << K) - 1u;
    kws_handle *h0 = kws_bank_member(b, 0);
    const size_t clip = (size_t)kws_clip_samples(h0), stride = (size_t)kws_frame_stride_samples(h0), slice = 4000, S = 5;
    std::vector<int16_t> pcm(400000, 3);
    Outputs o(b, 256);
    EI_IMPULSE_ERROR rc;
    auto refuse = [&](const char *what, EI_IMPULSE_ERROR code, int state_ok = 1) {
        printf("refuse %s %s %d %d | %s\n", name, what, (int)code, o.untouched() && state_ok, kws_last_error());
    };
    auto call = [&](const char *what, EI_IMPULSE_ERROR code) { printf("call %s %s %d\n", name, what, (int)code); };

    // ---- clips
    {
        const size_t B = 9;
        std::vector<uint32_t> all(B, every), onehot(B), first(B, 1u), last(B, 1u << (K - 1)), none(B, 0u), bad(B, every);
        for (size_t i = 0; i < B; i++) onehot[i] = 1u << (i % K);
        bad[3] = every | (1u << K);
        bad[5] = 1u << 20;
        { Section s(name, "routed_bad_bit"); refuse("routed_bad_bit", kws_bank_run_classifier_routed_device(b, pcm.data(), B, bad.data(), o.sp.data(), o.feats.data(), nullptr)); }
        { Section s(name, "routed_null_bank"); refuse("routed_null_bank", kws_bank_run_classifier_routed_device(nullptr, pcm.data(), B, onehot.data(), o.sp.data(), nullptr, nullptr)); }
        { Section s(name, "routed_null_pcm"); refuse("routed_null_pcm", kws_bank_run_classifier_routed_device(b, nullptr, B, onehot.data(), o.sp.data(), nullptr, nullptr)); }
        { Section s(name, "routed_null_scores"); refuse("routed_null_scores", kws_bank_run_classifier_routed_device(b, pcm.data(), B, onehot.data(), nullptr, o.feats.data(), nullptr)); }
        Outputs w(b, B);
        { Section s(name, "batch_unrouted"); call("batch_unrouted", kws_bank_run_classifier_batch_device(b, pcm.data(), B, w.sp.data(), w.feats.data(), nullptr)); }
        { Section s(name, "batch_null_routes"); call("batch_null_routes", kws_bank_run_classifier_routed_device(b, pcm.data(), B, nullptr, w.sp.data(), w.feats.data(), nullptr)); }
        { Section s(name, "batch_all_routes"); call("batch_all_routes", kws_bank_run_classifier_routed_device(b, pcm.data(), B, all.data(), w.sp.data(), w.feats.data(), nullptr)); }
        { Section s(name, "batch_onehot"); call("batch_onehot", kws_bank_run_classifier_routed_device(b, pcm.data(), B, onehot.data(), w.sp.data(), w.feats.data(), nullptr)); }
        { Section s(name, "batch_first_only"); call("batch_first_only", kws_bank_run_classifier_routed_device(b, pcm.data(), B, first.data(), w.sp.data(), nullptr, nullptr)); }
        { Section s(name, "batch_last_only"); call("batch_last_only", kws_bank_run_classifier_routed_device(b, pcm.data(), B, last.data(), w.sp.data(), nullptr, nullptr)); }
        { Section s(name, "batch_none"); call("batch_none", kws_bank_run_classifier_routed_device(b, pcm.data(), B, none.data(), w.sp.data(), w.feats.data(), nullptr)); }
        { Section s(name, "batch_b0"); call("batch_b0", kws_bank_run_classifier_routed_device(b, pcm.data(), 0, onehot.data(), w.sp.data(), w.feats.data(), nullptr)); }
    }

    // ---- clips of their own lengths
    {
        const size_t B = 6;
        const size_t offs[6] = { 0, 16008, 32017, 48001, 64000, 90003 }, lens[6] = { clip, 640, clip - 1, 5000, clip + stride - 1, 12345 };
        uint32_t all[6], onehot[6], bad[6];
        for (size_t i = 0; i < B; i++) { all[i] = every; onehot[i] = 1u << (i % K); bad[i] = every; }
        bad[4] = 1u << K;
        { Section s(name, "ragged_routed_bad_bit"); refuse("ragged_routed_bad_bit", kws_bank_run_classifier_ragged_routed_device(b, pcm.data(), offs, lens, B, bad, o.sp.data(), o.feats.data(), nullptr)); }
        { Section s(name, "ragged_routed_null_bank"); refuse("ragged_routed_null_bank", kws_bank_run_classifier_ragged_routed_device(nullptr, pcm.data(), offs, lens, B, onehot, o.sp.data(), nullptr, nullptr)); }
        { Section s(name, "ragged_routed_null_scores"); refuse("ragged_routed_null_scores", kws_bank_run_classifier_ragged_routed_device(b, pcm.data(), offs, lens, B, onehot, nullptr, o.feats.data(), nullptr)); }
        { Section s(name, "ragged_routed_null_pcm"); refuse("ragged_routed_null_pcm", kws_bank_run_classifier_ragged_routed_device(b, nullptr, offs, lens, B, onehot, o.sp.data(), nullptr, nullptr)); }
        Outputs w(b, B);
        { Section s(name, "ragged_unrouted"); call("ragged_unrouted", kws_bank_run_classifier_ragged_device(b, pcm.data(), offs, lens, B, w.sp.data(), w.feats.data(), nullptr)); }
        { Section s(name, "ragged_null_routes"); call("ragged_null_routes", kws_bank_run_classifier_ragged_routed_device(b, pcm.data(), offs, lens, B, nullptr, w.sp.data(), w.feats.data(), nullptr)); }
        { Section s(name, "ragged_all_routes"); call("ragged_all_routes", kws_bank_run_classifier_ragged_routed_device(b, pcm.data(), offs, lens, B, all, w.sp.data(), w.feats.data(), nullptr)); }
        { Section s(name, "ragged_onehot"); call("ragged_onehot", kws_bank_run_classifier_ragged_routed_device(b, pcm.data(), offs, lens, B, onehot, w.sp.data(), w.feats.data(), nullptr)); }
    }

    // ---- live continuous sessions
    {
        kws_bank_live *fresh = nullptr, *alls = nullptr, *hot = nullptr;
        if (kws_bank_live_create(b, S, slice, &fresh) || kws_bank_live_create(b, S, slice, &alls) || kws_bank_live_create(b, S, slice, &hot)) { call("live_create", (EI_IMPULSE_ERROR)-1); return; }
        const size_t every_stream[5] = { 0, 1, 2, 3, 4 };
        uint32_t all[5], onehot[5];
        for (size_t i = 0; i < S; i++) { all[i] = every; onehot[i] = 1u << (i % K); }
        const size_t st2[2] = { 0, 2 }, of2[2] = { 3, 70001 }, ln2[2] = { 3 * slice + 320, 6 * slice + 320 };
        const size_t st3[3] = { 0, 1, 2 }, of3[3] = { 3, 70001, 140001 }, ln3[3] = { 7 * slice + 320, 6 * slice + 320, 5 * slice + 320 };
        size_t nw[3];
        Outputs w(b, 64);
        { Section s(name, "live_push_fresh"); call("live_push_fresh", kws_bank_live_push_device(fresh, 3, st3, pcm.data(), of3, ln3, nullptr, w.sp.data(), w.rp.data(), nw, nullptr)); }
        call("live_route_all", kws_bank_live_route(alls, every_stream, S, all));
        { Section s(name, "live_push_all_routes"); call("live_push_all_routes", kws_bank_live_push_device(alls, 3, st3, pcm.data(), of3, ln3, nullptr, w.sp.data(), w.rp.data(), nw, nullptr)); }
        { Section s(name, "live_route_onehot"); call("live_route_onehot", kws_bank_live_route(hot, every_stream, S, onehot)); }
        {
            // streams 0, 1, 2 name members 0, 1 % K, 2 % K: a member none of them names may be skipped
            std::vector<float *> some(w.sp), some_raw(w.rp);
            for (size_t k = 0; k < K; k++)
                if (k != 0 && k != 1 % K && k != 2 % K) some[k] = some_raw[k] = nullptr;
            Section s(name, "live_push_onehot");
            call("live_push_onehot", kws_bank_live_push_device(hot, 3, st3, pcm.data(), of3, ln3, nullptr, some.data(), some_raw.data(), nw, nullptr));
        }
        // refusals: nothing changes -- stream 4 (not pushed to) keeps its route (member 4 % K) although the refused call names it first
        const size_t s40[2] = { 4, 0 }, far[1] = { S }, one4[1] = { 4 }, of1[1] = { 9 }, ln1[1] = { 5 * slice + 320 };
        const uint32_t other[2] = { (uint32_t)(1u << ((4 % K + 1) % K)), 0u }, badbit[1] = { (uint32_t)(1u << K) }, zero1[1] = { 0u };
        size_t before = 0, after = 0;
        (void)kws_bank_live_window_count(hot, 0, slice, 0, &before);
        auto same = [&]() { (void)kws_bank_live_window_count(hot, 0, slice, 0, &after); return after == before ? 1 : 0; };
        { Section s(name, "live_route_pushed"); rc = kws_bank_live_route(hot, s40, 2, other); refuse("live_route_pushed", rc, same()); }
        { Section s(name, "live_route_range"); rc = kws_bank_live_route(hot, far, 1, zero1); refuse("live_route_range", rc, same()); }
        { Section s(name, "live_route_bad_bit"); rc = kws_bank_live_route(hot, one4, 1, badbit); refuse("live_route_bad_bit", rc, same()); }
        { Section s(name, "live_route_null_session"); rc = kws_bank_live_route(nullptr, one4, 1, zero1); refuse("live_route_null_session", rc, same()); }
        { Section s(name, "live_route_null_routes"); rc = kws_bank_live_route(hot, one4, 1, nullptr); refuse("live_route_null_routes", rc, same()); }
        if (K > 1) {
            // stream 4 still routes to member 4 % K alone: that member's scores are needed, every other member's are not
            std::vector<float *> without(o.sp), only(K, nullptr);
            without[4 % K] = nullptr;
            size_t n1[1] = { 77 };
            { Section s(name, "live_push_needed_null"); rc = kws_bank_live_push_device(hot, 1, one4, pcm.data(), of1, ln1, nullptr, without.data(), nullptr, n1, nullptr); refuse("live_push_needed_null", rc, same() && n1[0] == 77); }
            only[4 % K] = w.sp[4 % K];
            { Section s(name, "live_push_only_needed"); call("live_push_only_needed", kws_bank_live_push_device(hot, 1, one4, pcm.data(), of1, ln1, nullptr, only.data(), nullptr, n1, nullptr)); }
        }
        // a reset keeps routes and lets them change again
        call("live_reset", kws_bank_live_reset(hot, st2, 1));
        call("live_route_after_reset", kws_bank_live_route(hot, st2, 1, zero1));
        {
            // stream 0 now names nobody: pushed alone, no member's scores are needed, and no network is launched
            std::vector<float *> nobody(K, nullptr);
            nobody[0] = w.sp[0];
            Section s(name, "live_push_unrouted_stream");
            call("live_push_unrouted_stream", kws_bank_live_push_device(hot, 1, st2, pcm.data(), of2, ln2, nullptr, nobody.data(), nullptr, nw, nullptr));
        }
        kws_bank_live_destroy(hot);
        kws_bank_live_destroy(alls);
        kws_bank_live_destroy(fresh);
    }

    // ---- live one-shot windows
    {
        kws_bank_slide_live *fresh = nullptr, *alls = nullptr, *hot = nullptr;
        const size_t hop = 5 * stride;
        if (kws_bank_slide_live_create(b, S, hop, 0, &fresh) || kws_bank_slide_live_create(b, S, hop, 0, &alls) || kws_bank_slide_live_create(b, S, hop, 0, &hot)) { call("slide_create", (EI_IMPULSE_ERROR)-1); return; }
        const size_t every_stream[5] = { 0, 1, 2, 3, 4 };
        uint32_t all[5], onehot[5], shifted[5];
        for (size_t i = 0; i < S; i++) { all[i] = every; onehot[i] = 1u << (i % K); shifted[i] = 1u << ((i + 1) % K); }
        const size_t st3[3] = { 4, 1, 2 }, of3[3] = { 5, 90001, 180001 }, ln3[3] = { clip + 3 * hop + 7, clip, clip + hop }, more[3] = { hop, hop, hop };
        size_t nw[3];
        Outputs w(b, 64);
        { Section s(name, "slide_push_fresh"); call("slide_push_fresh", kws_bank_slide_live_push_device(fresh, 3, st3, pcm.data(), of3, ln3, w.sp.data(), w.feats.data(), nw, nullptr)); }
        call("slide_route_all", kws_bank_slide_live_route(alls, every_stream, S, all));
        { Section s(name, "slide_push_all_routes"); call("slide_push_all_routes", kws_bank_slide_live_push_device(alls, 3, st3, pcm.data(), of3, ln3, w.sp.data(), w.feats.data(), nw, nullptr)); }
        call("slide_route_onehot", kws_bank_slide_live_route(hot, every_stream, S, onehot));
        { Section s(name, "slide_push_onehot"); call("slide_push_onehot", kws_bank_slide_live_push_device(hot, 3, st3, pcm.data(), of3, ln3, w.sp.data(), w.feats.data(), nw, nullptr)); }
        // a route may change between any two pushes
        { Section s(name, "slide_route_change"); call("slide_route_change", kws_bank_slide_live_route(hot, every_stream, S, shifted)); }
        { Section s(name, "slide_push_rerouted"); call("slide_push_rerouted", kws_bank_slide_live_push_device(hot, 3, st3, pcm.data(), of3, more, w.sp.data(), nullptr, nw, nullptr)); }
        const size_t far[1] = { S }, one4[1] = { 4 };
        const uint32_t badbit[1] = { (uint32_t)(1u << K) }, zero1[1] = { 0u };
        size_t before = 0, after = 0;
        (void)kws_bank_slide_live_window_count(hot, 4, hop, &before);
        auto same = [&]() { (void)kws_bank_slide_live_window_count(hot, 4, hop, &after); return after == before ? 1 : 0; };
        { Section s(name, "slide_route_range"); rc = kws_bank_slide_live_route(hot, far, 1, zero1); refuse("slide_route_range", rc, same()); }
        { Section s(name, "slide_route_bad_bit"); rc = kws_bank_slide_live_route(hot, one4, 1, badbit); refuse("slide_route_bad_bit", rc, same()); }
        { Section s(name, "slide_route_null_session"); rc = kws_bank_slide_live_route(nullptr, one4, 1, zero1); refuse("slide_route_null_session", rc, same()); }
        kws_bank_slide_live_destroy(fresh);
        kws_bank_slide_live_destroy(alls);
        kws_bank_slide_live_destroy(hot);
    }
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
    // list building as host arithmetic: random masks with zero masks among them, at the sizes' edges
    const size_t Ks[] = { 1, 2, 4, 7, 16 }, ns[] = { 0, 1, 37, 300 };
    unsigned seed = 99;
    for (size_t K : Ks)
        for (size_t n : ns) print_lists(K, n, seed++);
    kws_bank_destroy(b13);
    kws_bank_destroy(b1);
    kws_bank_destroy(b40);
    for (int i = 0; i < 7; i++) kws_destroy(h[i]);
    printf("done\n");
    return 0;
}
