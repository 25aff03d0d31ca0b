// slide_host_driver.cpp -- TEST INFRASTRUCTURE ONLY (tests/test_slide_host.py): the argument checks and the host arithmetic of
// kws_slide_window_count / kws_slide_plan / kws_slide_recordings_device, run against the stub HIP runtime of tests/sanitize (device memory =
// host heap, launches do nothing) under ASan + UBSan.  No value a kernel would write means anything here.
// usage: kws_slide_san model.kwsm ...   prints, per model:
//   model <path> rc <kws_create's code>
//   geom <clip> <frames> <stride>
//   count <n_samples> <hop> <windows> <code>
//   plan <hop> <flags> <code> <n_windows> <rows_shared> <rows_first> <rows_direct> <phases> <path>       over the lengths of LENS
//   hop0 | nullscores | badflags | nullpcm | hugelen | hugehop | hugecount <code>;  empty | short <code> <untouched>
//   full <mode> <flags> <hop> <code>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../include/kws/kws.h"

int main(int argc, char **argv)
{
    for (int i = 1; i < argc; i++) {
        kws_handle *h = nullptr;
        EI_IMPULSE_ERROR rc = kws_create_from_file(argv[i], 0, &h);
        printf("model %s rc %d\n", argv[i], (int)rc);
        if (rc) continue;
        const size_t C = (size_t)kws_label_count(h), F = (size_t)kws_feature_count(h), clip = (size_t)kws_clip_samples(h);
        const size_t stride = (size_t)kws_frame_stride_samples(h);
        printf("geom %zu %d %zu\n", clip, kws_frame_count(h), stride);
        const size_t hops[] = { stride, 2 * stride, 4000, 1000, 7, 1, clip, clip + 13 };
        const size_t LENS[] = { 0, clip - 1, clip, clip + 1, clip + stride - 1, clip + stride, clip + 3 * stride + 7, 3 * clip, clip + 60, 960000 };
        const size_t n_lens = sizeof(LENS) / sizeof(LENS[0]);
        for (size_t hop : hops) {
            for (size_t n : LENS) {
                size_t w = 12345;
                rc = kws_slide_window_count(h, n, hop, &w);
                printf("count %zu %zu %zu %d\n", n, hop, w, (int)rc);
            }
            for (int flags = 0; flags < 3; flags++) {
                kws_slide_plan_info I;
                memset(&I, 0xff, sizeof(I));
                rc = kws_slide_plan(h, LENS, n_lens, hop, flags, &I);
                printf("plan %zu %d %d %zu %zu %zu %zu %d %d\n", hop, flags, (int)rc, I.n_windows, I.rows_shared, I.rows_first, I.rows_direct, I.phases, I.path);
            }
        }
        std::vector<int16_t> pcm(200000, 3);
        std::vector<float> scores(64 * C, -7.0f), feats(64 * F, -7.0f);
        const size_t off1[1] = { 1 }, len1[1] = { clip + 5 * stride };
        size_t w = 0;
        kws_slide_plan_info I;
        printf("hop0 %d %d %d\n", (int)kws_slide_recordings_device(h, pcm.data(), off1, len1, 1, 0, 0, scores.data(), nullptr, nullptr),
               (int)kws_slide_window_count(h, clip, 0, &w), (int)kws_slide_plan(h, len1, 1, 0, 0, &I));
        printf("nullscores %d\n", (int)kws_slide_recordings_device(h, pcm.data(), off1, len1, 1, stride, 0, nullptr, feats.data(), nullptr));
        printf("badflags %d %d %d\n", (int)kws_slide_recordings_device(h, pcm.data(), off1, len1, 1, stride, 3, scores.data(), nullptr, nullptr),
               (int)kws_slide_recordings_device(h, pcm.data(), off1, len1, 1, stride, -1, scores.data(), nullptr, nullptr),
               (int)kws_slide_plan(h, len1, 1, stride, 7, &I));
        printf("nullpcm %d\n", (int)kws_slide_recordings_device(h, nullptr, off1, len1, 1, stride, 0, scores.data(), nullptr, nullptr));
        const size_t huge[1] = { (size_t)-1 - 5 };
        printf("hugelen %d %d %d\n", (int)kws_slide_window_count(h, huge[0], 1, &w), (int)kws_slide_plan(h, huge, 1, 1, 0, &I),
               (int)kws_slide_recordings_device(h, pcm.data(), off1, huge, 1, 1, 0, scores.data(), nullptr, nullptr));
        printf("hugehop %d\n", (int)kws_slide_window_count(h, clip, (size_t)-1, &w));
        const size_t many[2] = { (size_t)1 << 55, (size_t)1 << 55 };
        printf("hugecount %d\n", (int)kws_slide_plan(h, many, 2, 1, 0, &I));
        std::fill(scores.begin(), scores.end(), -7.0f);
        rc = kws_slide_recordings_device(h, pcm.data(), nullptr, nullptr, 0, stride, 0, scores.data(), feats.data(), nullptr);
        bool untouched = true;
        for (float v : scores) untouched = untouched && v == -7.0f;
        printf("empty %d %d\n", (int)rc, untouched ? 1 : 0);
        const size_t off2[3] = { 0, 5, 7 }, len2[3] = { clip - 1, 100, 0 };
        rc = kws_slide_recordings_device(h, pcm.data(), off2, len2, 3, stride, 0, scores.data(), feats.data(), nullptr);
        for (float v : scores) untouched = untouched && v == -7.0f;
        for (float v : feats) untouched = untouched && v == -7.0f;
        printf("short %d %d\n", (int)rc, untouched ? 1 : 0);
        // calls that do work (host logic only): recordings at odd offsets, one of them long enough for several chunks of staged items
        std::vector<int16_t> big(3000001, 5);
        const size_t off3[4] = { 1, 17, 40001, 123 }, len3[4] = { clip + 24000, clip + stride - 1, 2900000, clip };
        for (int mode = 0; mode < 2; mode++) {
            if (kws_set_mode(h, mode) != EI_IMPULSE_OK) continue;
            for (int flags = 0; flags < 3; flags++)
                for (size_t hop : hops) {
                    if (hop < 100 && flags != 2) continue;                 // (the small hops once: the windows of 3 minutes at hop 1 are many)
                    const size_t n_rec = hop < 100 ? 2 : 4;
                    if (kws_slide_plan(h, len3, n_rec, hop, flags, &I) != EI_IMPULSE_OK) { printf("full %d %d %zu %d\n", mode, flags, hop, -99); continue; }
                    std::vector<float> s2(I.n_windows * C), f2(mode ? 0 : I.n_windows * F);
                    rc = kws_slide_recordings_device(h, big.data(), off3, len3, n_rec, hop, flags, s2.data(), mode ? nullptr : f2.data(), nullptr);
                    size_t nfb = 0;
                    (void)kws_fast_fallback_count(h, &nfb);
                    printf("full %d %d %zu %d\n", mode, flags, hop, (int)rc);
                }
        }
        kws_destroy(h);
    }
    return 0;
}
