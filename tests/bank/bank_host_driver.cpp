// bank_host_driver.cpp -- TEST INFRASTRUCTURE ONLY (tests/test_bank_host.py): membership rules, argument checks and the host bookkeeping of
// kws_bank_* run against the stub HIP runtime of tests/sanitize (device memory = host heap, launches do nothing) under ASan + UBSan.
// No value a kernel would write means anything here.
// usage: kws_bank_san mfcc40_a mfcc40_b mfcc40_c mfcc40_d l476 l476_f32 l432      prints
//   load <n> <code>                          per model
//   create <name> <code> <size> <members in order: 1/0>
//   refuse <name> <code> <out pointer left NULL: 1/0> <kws_last_error text>
//   usable <name> <code>                     a member's own batch call after the refusals
//   args <bank> <name> <code>                argument checks of the three calls
//   empty <bank> <name> <code> <untouched>   calls that must write nothing
//   call <bank> <name> <code>                calls that do work
//   slide <bank> <flags> <hop> <code>
//   done
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../include/kws/kws.h"

static bool all_are(const std::vector<float> &v, float x)
{
    for (float f : v) if (f != x) return false;
    return true;
}

static void exercise(const char *name, kws_bank *b)
{
    const size_t K = kws_bank_size(b);
    kws_handle *h0 = kws_bank_member(b, 0);
    const size_t F = (size_t)kws_feature_count(h0), clip = (size_t)kws_clip_samples(h0), stride = (size_t)kws_frame_stride_samples(h0);
    const size_t B = 9;
    std::vector<int16_t> pcm(B * clip + 64, 3);
    std::vector<float> cep(B * F, 0.5f), feats(64 * F, -7.0f);
    std::vector<std::vector<float>> sc(K);
    std::vector<float *> sp(K), none(K, nullptr);
    for (size_t k = 0; k < K; k++) {
        sc[k].assign(64 * (size_t)kws_label_count(kws_bank_member(b, k)), -7.0f);
        sp[k] = sc[k].data();
    }
    const size_t off1[1] = { 1 }, len1[1] = { clip + 5 * stride };
    // ---- argument checks
    printf("args %s null_bank %d\n", name, (int)kws_bank_run_classifier_batch_device(nullptr, pcm.data(), B, sp.data(), nullptr, nullptr));
    printf("args %s null_pcm %d\n", name, (int)kws_bank_run_classifier_batch_device(b, nullptr, B, sp.data(), nullptr, nullptr));
    printf("args %s null_scores %d\n", name, (int)kws_bank_run_classifier_batch_device(b, pcm.data(), B, nullptr, feats.data(), nullptr));
    printf("args %s nothing_wanted %d\n", name, (int)kws_bank_run_classifier_batch_device(b, pcm.data(), B, none.data(), nullptr, nullptr));
    printf("args %s huge_batch %d\n", name, (int)kws_bank_run_classifier_batch_device(b, pcm.data(), (size_t)1 << 31, sp.data(), nullptr, nullptr));
    printf("args %s cmvn_null_mfcc %d\n", name, (int)kws_bank_cmvn_inference_batch_device(b, nullptr, B, sp.data(), nullptr, nullptr));
    printf("args %s cmvn_nothing_wanted %d\n", name, (int)kws_bank_cmvn_inference_batch_device(b, cep.data(), B, none.data(), nullptr, nullptr));
    printf("args %s cmvn_null_bank %d\n", name, (int)kws_bank_cmvn_inference_batch_device(nullptr, cep.data(), B, sp.data(), nullptr, nullptr));
    printf("args %s slide_hop0 %d\n", name, (int)kws_bank_slide_recordings_device(b, pcm.data(), off1, len1, 1, 0, 0, sp.data(), nullptr, nullptr));
    printf("args %s slide_badflags %d\n", name, (int)kws_bank_slide_recordings_device(b, pcm.data(), off1, len1, 1, stride, 3, sp.data(), nullptr, nullptr));
    printf("args %s slide_null_pcm %d\n", name, (int)kws_bank_slide_recordings_device(b, nullptr, off1, len1, 1, stride, 0, sp.data(), nullptr, nullptr));
    printf("args %s slide_null_scores %d\n", name, (int)kws_bank_slide_recordings_device(b, pcm.data(), off1, len1, 1, stride, 0, nullptr, feats.data(), nullptr));
    printf("args %s slide_nothing_wanted %d\n", name, (int)kws_bank_slide_recordings_device(b, pcm.data(), off1, len1, 1, stride, 0, none.data(), nullptr, nullptr));
    const size_t huge[1] = { (size_t)-1 - 5 };
    printf("args %s slide_hugelen %d\n", name, (int)kws_bank_slide_recordings_device(b, pcm.data(), off1, huge, 1, 1, 0, sp.data(), nullptr, nullptr));
    printf("args %s member_past_end %d\n", name, kws_bank_member(b, K) == nullptr ? -20 : 0);
    // ---- calls that must write nothing (the stub's device memory is the host's: a write would show)
    auto untouched = [&]() {
        bool ok = all_are(feats, -7.0f);
        for (size_t k = 0; k < K; k++) ok = ok && all_are(sc[k], -7.0f);
        return ok ? 1 : 0;
    };
    EI_IMPULSE_ERROR rc = kws_bank_run_classifier_batch_device(b, pcm.data(), 0, sp.data(), feats.data(), nullptr);
    printf("empty %s batch0 %d %d\n", name, (int)rc, untouched());
    rc = kws_bank_cmvn_inference_batch_device(b, cep.data(), 0, sp.data(), feats.data(), nullptr);
    printf("empty %s cmvn0 %d %d\n", name, (int)rc, untouched());
    rc = kws_bank_slide_recordings_device(b, pcm.data(), nullptr, nullptr, 0, stride, 0, sp.data(), feats.data(), nullptr);
    printf("empty %s slide_r0 %d %d\n", name, (int)rc, untouched());
    const size_t off2[3] = { 0, 5, 7 }, len2[3] = { clip - 1, 100, 0 };
    rc = kws_bank_slide_recordings_device(b, pcm.data(), off2, len2, 3, stride, 0, sp.data(), feats.data(), nullptr);
    printf("empty %s slide_short %d %d\n", name, (int)rc, untouched());
    // ---- calls that do work: every member, a subset, features only, with and without the caller's feature buffer (the bank's grows)
    std::vector<float *> some(sp);
    if (K > 1) some[0] = nullptr;
    printf("call %s batch %d\n", name, (int)kws_bank_run_classifier_batch_device(b, pcm.data(), B, sp.data(), feats.data(), nullptr));
    printf("call %s batch_own_buffer %d\n", name, (int)kws_bank_run_classifier_batch_device(b, pcm.data(), B, sp.data(), nullptr, nullptr));
    printf("call %s batch_subset %d\n", name, (int)kws_bank_run_classifier_batch_device(b, pcm.data(), B - 4, some.data(), nullptr, nullptr));
    printf("call %s batch_features_only %d\n", name, (int)kws_bank_run_classifier_batch_device(b, pcm.data(), B, none.data(), feats.data(), nullptr));
    printf("call %s cmvn %d\n", name, (int)kws_bank_cmvn_inference_batch_device(b, cep.data(), B, sp.data(), feats.data(), nullptr));
    printf("call %s cmvn_own_buffer %d\n", name, (int)kws_bank_cmvn_inference_batch_device(b, cep.data(), B, some.data(), nullptr, nullptr));
    // a member in fast mode: bank calls neither follow nor change it
    kws_handle *hl = kws_bank_member(b, K - 1);
    const bool fast = kws_set_mode(hl, KWS_MODE_FAST) == EI_IMPULSE_OK;
    printf("call %s batch_member_fast %d\n", name, (int)kws_bank_run_classifier_batch_device(b, pcm.data(), B, sp.data(), nullptr, nullptr));
    printf("call %s mode_kept %d\n", name, kws_get_mode(hl) == (fast ? KWS_MODE_FAST : KWS_MODE_EXACT) ? 0 : -1);
    (void)kws_set_mode(hl, KWS_MODE_EXACT);
    // the slide on every path: recordings at odd offsets, one long enough for several chunks of staged items, one too short
    std::vector<int16_t> big(3000001, 5);
    const size_t off3[4] = { 1, 17, 40001, 123 }, len3[4] = { clip + 24000, clip - 1, 2900000, clip };
    const size_t hops[] = { stride, 1600, 1000, clip + 13 };
    for (int flags = 0; flags < 3; flags++)
        for (size_t hop : hops) {
            kws_slide_plan_info I;
            if (kws_slide_plan(h0, len3, 4, hop, flags, &I) != EI_IMPULSE_OK) { printf("slide %s %d %zu %d\n", name, flags, hop, -99); continue; }
            std::vector<std::vector<float>> s2(K);
            std::vector<float *> p2(K);
            for (size_t k = 0; k < K; k++) {
                s2[k].resize(I.n_windows * (size_t)kws_label_count(kws_bank_member(b, k)));
                p2[k] = s2[k].data();
            }
            std::vector<float> f2(hop == 1600 ? I.n_windows * F : 0);
            rc = kws_bank_slide_recordings_device(b, big.data(), off3, len3, 4, hop, flags, p2.data(), f2.empty() ? nullptr : f2.data(), nullptr);
            printf("slide %s %d %zu %d\n", name, flags, hop, (int)rc);
        }
}

int main(int argc, char **argv)
{
    if (argc != 8) { fprintf(stderr, "usage: %s mfcc40 x 4, l476, l476_f32, l432\n", argv[0]); return 2; }
    kws_handle *h[7] = { nullptr };
    for (int i = 0; i < 7; i++) printf("load %d %d\n", i, (int)kws_create_from_file(argv[i + 1], 0, &h[i]));
    for (int i = 0; i < 7; i++) if (!h[i]) return 1;
    kws_handle *l476 = h[4], *l476f = h[5], *l432 = h[6];

    auto refuse = [&](const char *name, kws_handle *const *m, size_t K) {
        kws_bank *b = (kws_bank *)(uintptr_t)0x10;           // must be overwritten with NULL
        const EI_IMPULSE_ERROR rc = kws_bank_create(m, K, &b);
        printf("refuse %s %d %d %s\n", name, (int)rc, b == nullptr ? 1 : 0, rc ? kws_last_error() : "-");
        if (rc == EI_IMPULSE_OK) kws_bank_destroy(b);
    };
    {
        kws_handle *m[2] = { l476, l432 };
        refuse("l476_l432", m, 2);
        refuse("k0", m, 0);
        kws_handle *many[17];
        for (int i = 0; i < 17; i++) many[i] = l476;
        refuse("k17", many, 17);
        kws_handle *withnull[3] = { l476, nullptr, l476f };
        refuse("null_member", withnull, 3);
        kws_handle *twice[3] = { l476, l476f, l476 };
        refuse("twice", twice, 3);
        kws_handle *mixed[2] = { h[0], l476 };
        refuse("mfcc40_l476", mixed, 2);
        kws_bank *b = nullptr;
        printf("refuse null_out %d 1 %s\n", (int)kws_bank_create(m, 2, nullptr), kws_last_error());
        printf("refuse null_members %d %d %s\n", (int)kws_bank_create(nullptr, 2, &b), b == nullptr ? 1 : 0, kws_last_error());
    }
    // the members are as usable as before
    {
        const size_t clip = (size_t)kws_clip_samples(l476);
        std::vector<int16_t> pcm(4 * clip, 3);
        kws_handle *m[3] = { l476, l476f, l432 };
        const char *names[3] = { "l476", "l476_f32", "l432" };
        for (int i = 0; i < 3; i++) {
            std::vector<float> s(4 * (size_t)kws_label_count(m[i]));
            printf("usable %s %d\n", names[i], (int)kws_run_classifier_batch_device(m[i], pcm.data(), 4, s.data(), nullptr, nullptr, nullptr));
        }
    }
    kws_bank *b40 = nullptr, *b13 = nullptr, *b13r = nullptr, *b1 = nullptr;
    EI_IMPULSE_ERROR rc = kws_bank_create(h, 4, &b40);
    printf("create mfcc40 %d %zu %d\n", (int)rc, kws_bank_size(b40),
           b40 && kws_bank_member(b40, 0) == h[0] && kws_bank_member(b40, 1) == h[1] && kws_bank_member(b40, 2) == h[2] && kws_bank_member(b40, 3) == h[3]);
    kws_handle *pair[2] = { l476, l476f }, *riap[2] = { l476f, l476 };
    rc = kws_bank_create(pair, 2, &b13);
    printf("create l476 %d %zu %d\n", (int)rc, kws_bank_size(b13), b13 && kws_bank_member(b13, 0) == l476 && kws_bank_member(b13, 1) == l476f);
    // a second bank over the same handles in the other order, and a bank of one
    rc = kws_bank_create(riap, 2, &b13r);
    printf("create l476_reversed %d %zu %d\n", (int)rc, kws_bank_size(b13r), b13r && kws_bank_member(b13r, 0) == l476f && kws_bank_member(b13r, 1) == l476);
    rc = kws_bank_create(&l432, 1, &b1);
    printf("create l432_alone %d %zu %d\n", (int)rc, kws_bank_size(b1), b1 && kws_bank_member(b1, 0) == l432);
    if (!b40 || !b13 || !b13r || !b1) return 1;
    exercise("mfcc40", b40);
    exercise("l476", b13);
    exercise("l476_reversed", b13r);
    exercise("l432_alone", b1);
    printf("size_null %zu\n", kws_bank_size(nullptr));
    // banks before their members
    kws_bank_destroy(b40);
    kws_bank_destroy(b13);
    kws_bank_destroy(b13r);
    kws_bank_destroy(b1);
    kws_bank_destroy(nullptr);
    for (int i = 0; i < 7; i++) kws_destroy(h[i]);
    printf("done\n");
    return 0;
}
