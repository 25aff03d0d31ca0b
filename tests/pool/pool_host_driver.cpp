// pool_host_driver.cpp -- TEST INFRASTRUCTURE ONLY (tests/test_pool_host.py): argument checks, list and work-item building and the host
// bookkeeping of the pool calls (kws_pool_*) run against the stub HIP runtime of tests/sanitize (device memory = host heap, launches do
// nothing) under ASan + UBSan.  No value a kernel would write means anything here.  With KWS_STUB_RECORD set the stub records every launch;
// the driver brackets each call it wants counted with "BEGIN <pool> <name>" / "END" notes.
// usage: kws_pool_san tenant40 x 6, tenant13, float32 twin of the 49x40 front end, DS-CNN of the 49x40 front end      prints
//   load <n> <code>
//   refuse <pool> <name> <code> <outputs and session state untouched: 1/0> | <kws_last_error>     (recorded: must launch nothing)
//   call <pool> <name> <code>                                                                    (recorded)
//   items <K> <n> <item_rows> | <member ...> | <the items, 4 ints each ...> | <the packed row list ...>
//   item_rows <kws_pool_item_rows()>
//   done
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../include/kws/kws.h"

extern "C" void kws_stub_note(const char *line);
// the library's list and item builder (csrc/kws_pool.h; internal, linked statically here)
size_t kws_pool_items(const uint32_t *member, size_t n, size_t K, int item_rows, std::vector<int> &out, std::vector<int> &fill);

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
    Outputs(kws_pool *p, size_t rows)
        : sc(rows * kws_pool_score_stride(p), FILL), raw(rows * kws_pool_score_stride(p), FILL), feats(rows * (size_t)kws_feature_count(kws_pool_member(p, 0)), FILL)
    {
    }
    int untouched() const { return all_are(sc, FILL) && all_are(raw, FILL) && all_are(feats, FILL) ? 1 : 0; }
};

static unsigned rnd(unsigned &s) { s = s * 1664525u + 1013904223u; return s >> 8; }

static void print_items(size_t K, size_t n, int item_rows, unsigned seed)
{
    std::vector<uint32_t> member(n);
    unsigned s = seed;
    // a quarter of the rows name nobody; half of the others name member 0, so that its list spans items at every item size
    for (size_t i = 0; i < n; i++) member[i] = rnd(s) % 4 == 0 ? KWS_POOL_NONE : rnd(s) % 2 == 0 ? 0u : (uint32_t)(rnd(s) % K);
    std::vector<int> out, fill;
    const size_t n_items = kws_pool_items(member.data(), n, K, item_rows, out, fill);
    printf("items %zu %zu %d |", K, n, item_rows);
    for (uint32_t m : member) printf(" %u", m);
    printf(" |");
    for (size_t i = 0; i < 4 * n_items; i++) printf(" %d", out[i]);
    printf(" |");
    for (size_t i = 4 * n_items; i < out.size(); i++) printf(" %d", out[i]);
    printf("\n");
}

static void creation(kws_handle **t40, kws_handle *t13, kws_handle *f32, kws_handle *dscnn)
{
    kws_pool *p = (kws_pool *)(void *)&p;            // (a refusal must reset it)
    auto refuse = [&](const char *what, EI_IMPULSE_ERROR code) {
        printf("refuse create %s %d %d | %s\n", what, (int)code, p == nullptr ? 1 : 0, kws_last_error());
        p = (kws_pool *)(void *)&p;
    };
    // (K out of range: refused before a member is read -- the array holds six handles)
    { Section s("create", "k_zero"); refuse("k_zero", kws_pool_create(t40, 0, &p)); }
    { Section s("create", "k_above_max"); refuse("k_above_max", kws_pool_create(t40, (size_t)KWS_POOL_MAX + 1, &p)); }
    { Section s("create", "null_members"); refuse("null_members", kws_pool_create(nullptr, 3, &p)); }
    kws_handle *with_null[3] = { t40[0], nullptr, t40[2] }, *twice[4] = { t40[0], t40[1], t40[2], t40[1] }, *other[2] = { t40[0], t13 };
    kws_handle *with_float[3] = { t40[0], t40[1], f32 }, *with_dscnn[2] = { t40[0], dscnn }, *float_first[1] = { f32 };
    { Section s("create", "null_member"); refuse("null_member", kws_pool_create(with_null, 3, &p)); }
    { Section s("create", "same_handle_twice"); refuse("same_handle_twice", kws_pool_create(twice, 4, &p)); }
    { Section s("create", "other_front_end"); refuse("other_front_end", kws_pool_create(other, 2, &p)); }
    { Section s("create", "float32_member"); refuse("float32_member", kws_pool_create(with_float, 3, &p)); }
    { Section s("create", "float32_alone"); refuse("float32_alone", kws_pool_create(float_first, 1, &p)); }
    { Section s("create", "other_family_member"); refuse("other_family_member", kws_pool_create(with_dscnn, 2, &p)); }
    printf("refuse create null_out %d 1 | %s\n", (int)kws_pool_create(t40, 3, nullptr), kws_last_error());
}

static void exercise(const char *name, kws_pool *p)
{
    const size_t K = kws_pool_size(p);
    kws_handle *h0 = kws_pool_member(p, 0);
    const size_t clip = (size_t)kws_clip_samples(h0), stride = (size_t)kws_frame_stride_samples(h0), slice = 4000, S = 5;
    std::vector<int16_t> pcm(400000, 3);
    Outputs o(p, 256);
    EI_IMPULSE_ERROR rc;
    auto refuse = [&](const char *what, EI_IMPULSE_ERROR code, int state_ok = 1) {
        printf("refuse %s %s %d %d | %s\n", name, what, (int)code, o.untouched() && state_ok, kws_last_error());
    };
    auto call = [&](const char *what, EI_IMPULSE_ERROR code) { printf("call %s %s %d\n", name, what, (int)code); };
    printf("pool %s %zu %zu\n", name, K, kws_pool_score_stride(p));

    // ---- clips
    {
        const size_t B = 9;
        std::vector<uint32_t> robin(B), one(B, (uint32_t)(K - 1)), none(B, KWS_POOL_NONE), bad(B);
        for (size_t i = 0; i < B; i++) robin[i] = bad[i] = (uint32_t)(i % K);
        bad[3] = (uint32_t)K;
        bad[5] = (uint32_t)K + 7u;
        { Section s(name, "bad_index"); refuse("bad_index", kws_pool_run_classifier_device(p, pcm.data(), B, bad.data(), o.sc.data(), o.feats.data(), nullptr)); }
        { Section s(name, "no_output"); refuse("no_output", kws_pool_run_classifier_device(p, pcm.data(), B, robin.data(), nullptr, nullptr, nullptr)); }
        { Section s(name, "null_pool"); refuse("null_pool", kws_pool_run_classifier_device(nullptr, pcm.data(), B, robin.data(), o.sc.data(), nullptr, nullptr)); }
        { Section s(name, "null_pcm"); refuse("null_pcm", kws_pool_run_classifier_device(p, nullptr, B, robin.data(), o.sc.data(), nullptr, nullptr)); }
        { Section s(name, "null_member"); refuse("null_member", kws_pool_run_classifier_device(p, pcm.data(), B, nullptr, o.sc.data(), nullptr, nullptr)); }
        { Section s(name, "batch_too_large"); refuse("batch_too_large", kws_pool_run_classifier_device(p, pcm.data(), (size_t)1 << 31, robin.data(), o.sc.data(), nullptr, nullptr)); }
        Outputs w(p, B);
        std::vector<float> own(B * (size_t)kws_label_count(h0), FILL);
        { Section s(name, "own_batch"); call("own_batch", kws_run_classifier_batch_device(h0, pcm.data(), B, own.data(), w.feats.data(), nullptr, nullptr)); }
        { Section s(name, "batch_robin"); call("batch_robin", kws_pool_run_classifier_device(p, pcm.data(), B, robin.data(), w.sc.data(), w.feats.data(), nullptr)); }
        { Section s(name, "batch_one"); call("batch_one", kws_pool_run_classifier_device(p, pcm.data(), B, one.data(), w.sc.data(), nullptr, nullptr)); }
        { Section s(name, "batch_none"); call("batch_none", kws_pool_run_classifier_device(p, pcm.data(), B, none.data(), w.sc.data(), w.feats.data(), nullptr)); }
        { Section s(name, "batch_features_only"); call("batch_features_only", kws_pool_run_classifier_device(p, pcm.data(), B, robin.data(), nullptr, w.feats.data(), nullptr)); }
        { Section s(name, "batch_b0"); call("batch_b0", kws_pool_run_classifier_device(p, pcm.data(), 0, nullptr, w.sc.data(), w.feats.data(), nullptr)); }
    }

    // ---- clips of their own lengths
    {
        const size_t B = 6;
        const size_t offs[6] = { 0, 16008, 32017, 48001, 64000, 90003 }, lens[6] = { clip, 640, clip - 1, 5000, clip + stride - 1, 12345 };
        uint32_t robin[6], bad[6];
        for (size_t i = 0; i < B; i++) robin[i] = bad[i] = (uint32_t)(i % K);
        bad[4] = (uint32_t)K;
        { Section s(name, "ragged_bad_index"); refuse("ragged_bad_index", kws_pool_run_classifier_ragged_device(p, pcm.data(), offs, lens, B, bad, o.sc.data(), o.feats.data(), nullptr)); }
        { Section s(name, "ragged_null_pool"); refuse("ragged_null_pool", kws_pool_run_classifier_ragged_device(nullptr, pcm.data(), offs, lens, B, robin, o.sc.data(), nullptr, nullptr)); }
        { Section s(name, "ragged_no_output"); refuse("ragged_no_output", kws_pool_run_classifier_ragged_device(p, pcm.data(), offs, lens, B, robin, nullptr, nullptr, nullptr)); }
        { Section s(name, "ragged_null_member"); refuse("ragged_null_member", kws_pool_run_classifier_ragged_device(p, pcm.data(), offs, lens, B, nullptr, o.sc.data(), nullptr, nullptr)); }
        { Section s(name, "ragged_null_pcm"); refuse("ragged_null_pcm", kws_pool_run_classifier_ragged_device(p, nullptr, offs, lens, B, robin, o.sc.data(), nullptr, nullptr)); }
        { Section s(name, "ragged_null_lengths"); refuse("ragged_null_lengths", kws_pool_run_classifier_ragged_device(p, pcm.data(), offs, nullptr, B, robin, o.sc.data(), nullptr, nullptr)); }
        Outputs w(p, B);
        std::vector<float> own(B * (size_t)kws_label_count(h0), FILL);
        { Section s(name, "own_ragged"); call("own_ragged", kws_run_classifier_ragged_device(h0, pcm.data(), offs, lens, B, own.data(), w.feats.data(), nullptr, nullptr)); }
        { Section s(name, "ragged_robin"); call("ragged_robin", kws_pool_run_classifier_ragged_device(p, pcm.data(), offs, lens, B, robin, w.sc.data(), w.feats.data(), nullptr)); }
    }

    // ---- live continuous sessions
    {
        kws_live *own = nullptr;
        kws_pool_live *fresh = nullptr, *hot = nullptr;
        if (kws_live_create(h0, S, slice, &own) || kws_pool_live_create(p, S, slice, &fresh) || kws_pool_live_create(p, S, slice, &hot)) { call("live_create", (EI_IMPULSE_ERROR)-1); return; }
        const size_t every_stream[5] = { 0, 1, 2, 3, 4 };
        uint32_t robin[5];
        for (size_t i = 0; i < S; i++) robin[i] = (uint32_t)(i % K);
        const size_t st3[3] = { 0, 1, 2 }, of3[3] = { 3, 70001, 140001 }, ln3[3] = { 7 * slice + 320, 6 * slice + 320, 5 * slice + 320 };
        size_t nw[3] = { 0, 0, 0 };
        Outputs w(p, 64);
        std::vector<float> own_sc(64 * (size_t)kws_label_count(h0), FILL), own_raw(own_sc);
        { Section s(name, "own_live_push"); call("own_live_push", kws_live_push_device(own, 3, st3, pcm.data(), of3, ln3, nullptr, own_sc.data(), own_raw.data(), nw, nullptr)); }
        // a fresh session assigns every stream to nobody: the windows are counted, no network runs
        { Section s(name, "live_push_unassigned"); call("live_push_unassigned", kws_pool_live_push_device(fresh, 3, st3, pcm.data(), of3, ln3, nullptr, w.sc.data(), w.raw.data(), nw, nullptr)); }
        printf("windows %s unassigned %zu %zu %zu\n", name, nw[0], nw[1], nw[2]);
        { Section s(name, "live_assign"); call("live_assign", kws_pool_live_assign(hot, every_stream, S, robin)); }
        { Section s(name, "live_push_assigned"); call("live_push_assigned", kws_pool_live_push_device(hot, 3, st3, pcm.data(), of3, ln3, nullptr, w.sc.data(), w.raw.data(), nw, nullptr)); }
        printf("windows %s assigned %zu %zu %zu\n", name, nw[0], nw[1], nw[2]);
        { Section s(name, "live_push_in_place"); call("live_push_in_place", kws_pool_live_push_device(hot, 3, st3, pcm.data(), of3, ln3, nullptr, w.sc.data(), nullptr, nw, nullptr)); }
        // refusals: nothing changes -- stream 4 (not pushed to) keeps its member although the refused call names it first
        const size_t s40[2] = { 4, 0 }, s44[2] = { 4, 4 }, far[1] = { S }, one4[1] = { 4 }, of1[1] = { 9 }, ln1[1] = { 5 * slice + 320 }, s33[2] = { 3, 3 }, of2[2] = { 9, 50001 },
                     ln2[2] = { slice, slice };
        const uint32_t other[2] = { (uint32_t)((4 % K + 1) % K), KWS_POOL_NONE }, badidx[1] = { (uint32_t)K }, none1[1] = { KWS_POOL_NONE };
        size_t before = 0, after = 0, n1[2] = { 77, 77 };
        (void)kws_pool_live_window_count(hot, 0, slice, 0, &before);
        auto same = [&]() { (void)kws_pool_live_window_count(hot, 0, slice, 0, &after); return after == before ? 1 : 0; };
        { Section s(name, "assign_pushed"); rc = kws_pool_live_assign(hot, s40, 2, other); refuse("assign_pushed", rc, same()); }
        { Section s(name, "assign_range"); rc = kws_pool_live_assign(hot, far, 1, none1); refuse("assign_range", rc, same()); }
        { Section s(name, "assign_twice"); rc = kws_pool_live_assign(hot, s44, 2, other); refuse("assign_twice", rc, same()); }
        { Section s(name, "assign_bad_index"); rc = kws_pool_live_assign(hot, one4, 1, badidx); refuse("assign_bad_index", rc, same()); }
        { Section s(name, "assign_null_session"); rc = kws_pool_live_assign(nullptr, one4, 1, none1); refuse("assign_null_session", rc, same()); }
        { Section s(name, "assign_null_member"); rc = kws_pool_live_assign(hot, one4, 1, nullptr); refuse("assign_null_member", rc, same()); }
        { Section s(name, "push_stream_range"); rc = kws_pool_live_push_device(hot, 1, far, pcm.data(), of1, ln1, nullptr, o.sc.data(), nullptr, n1, nullptr); refuse("push_stream_range", rc, same() && n1[0] == 77); }
        { Section s(name, "push_stream_twice"); rc = kws_pool_live_push_device(hot, 2, s33, pcm.data(), of2, ln2, nullptr, o.sc.data(), nullptr, n1, nullptr); refuse("push_stream_twice", rc, same() && n1[0] == 77); }
        { Section s(name, "push_null_scores"); rc = kws_pool_live_push_device(hot, 1, one4, pcm.data(), of1, ln1, nullptr, nullptr, nullptr, n1, nullptr); refuse("push_null_scores", rc, same() && n1[0] == 77); }
        { Section s(name, "push_null_session"); rc = kws_pool_live_push_device(nullptr, 1, one4, pcm.data(), of1, ln1, nullptr, o.sc.data(), nullptr, n1, nullptr); refuse("push_null_session", rc, same()); }
        // stream 4 still has its member: pushed alone, one network launch; a reset keeps members and lets them change again
        { Section s(name, "live_push_stream4"); call("live_push_stream4", kws_pool_live_push_device(hot, 1, one4, pcm.data(), of1, ln1, nullptr, w.sc.data(), nullptr, n1, nullptr)); }
        call("live_reset", kws_pool_live_reset(hot, st3, 1));
        call("live_assign_after_reset", kws_pool_live_assign(hot, st3, 1, none1));
        { Section s(name, "live_push_after_unassign"); call("live_push_after_unassign", kws_pool_live_push_device(hot, 1, st3, pcm.data(), of3, ln3, nullptr, w.sc.data(), nullptr, nw, nullptr)); }
        // the push that finishes a stream puts it in its start state
        const int fin1[1] = { 1 };
        call("live_push_finish", kws_pool_live_push_device(hot, 1, one4, pcm.data(), of1, ln1, fin1, w.sc.data(), nullptr, n1, nullptr));
        call("live_assign_after_finish", kws_pool_live_assign(hot, one4, 1, none1));
        kws_pool_live_destroy(hot);
        kws_pool_live_destroy(fresh);
        kws_live_destroy(own);
    }
}

int main(int argc, char **argv)
{
    if (argc != 10) { fprintf(stderr, "usage: %s tenant40 x 6, tenant13, f32, dscnn\n", argv[0]); return 2; }
    kws_handle *h[9] = { nullptr };
    for (int i = 0; i < 9; i++) printf("load %d %d\n", i, (int)kws_create_from_file(argv[i + 1], 0, &h[i]));
    for (int i = 0; i < 9; i++) if (!h[i]) return 1;
    creation(h, h[6], h[7], h[8]);
    kws_pool *p6 = nullptr, *p1 = nullptr;
    if (kws_pool_create(h, 6, &p6) || kws_pool_create(&h[2], 1, &p1)) { fprintf(stderr, "%s\n", kws_last_error()); return 1; }
    printf("accessors %zu %d %d %zu %zu\n", kws_pool_size(p6), kws_pool_member(p6, 5) == h[5], kws_pool_member(p6, 6) == nullptr, kws_pool_size(nullptr), kws_pool_score_stride(nullptr));
    exercise("six", p6);
    exercise("alone", p1);
    // list and item building as host arithmetic: seeded members with rows that name nobody among them, at the sizes' and the item size's edges
    const size_t Ks[] = { 1, 3, 17, 40 }, ns[] = { 0, 1, 37, 300 };
    const int item_rows[] = { 4, 16, 64 };
    unsigned seed = 99;
    for (size_t K : Ks)
        for (size_t n : ns)
            for (int r : item_rows) print_items(K, n, r, seed++);
    printf("item_rows %d\n", kws_pool_item_rows());
    kws_pool_destroy(p1);
    kws_pool_destroy(p6);
    for (int i = 0; i < 9; i++) kws_destroy(h[i]);
    printf("done\n");
    return 0;
}
