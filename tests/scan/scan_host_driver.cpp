// scan_host_driver.cpp -- TEST INFRASTRUCTURE ONLY (tests/test_scan_host.py): the argument checks and the host arithmetic of
// kws_scan_window_count / kws_scan_recordings_device, run against the stub HIP runtime of tests/sanitize (device memory = host heap,
// launches do nothing) under ASan + UBSan.  No value a kernel would write means anything here.
// usage: kws_scan_san model.kwsm ...   prints, per model:
//   model <path> rc <kws_create's code>
//   count <n_samples> <windows>                      4000-sample slices
//   slicing <slice> <scan code> <stream code> <window-count code>     stream code: the first failing step of a fresh S = 1 batch (0: none)
//   null <code> | empty <code> <untouched> | short <code> <untouched> | full <mode> <code>
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
        const size_t C = (size_t)kws_label_count(h);
        const size_t lens[] = { 0, 3999, 4000, 15999, 16000, 16001, 19999, 20000, 24000, 960000, 57600000 };
        for (size_t n : lens) {
            size_t w = 12345;
            rc = kws_scan_window_count(h, n, 4000, &w);
            printf("count %zu %zu %d\n", n, w, (int)rc);
        }
        std::vector<int16_t> pcm(200000, 3);
        std::vector<float> scores(64 * C, -7.0f), raw(64 * C, -7.0f);
        const size_t slicings[] = { 4000, 4001, 100, 0, 8000, 16000, 3200 };
        for (size_t sl : slicings) {
            const size_t off[1] = { 1 }, len[1] = { 40000 };
            const int scan_rc = (int)kws_scan_recordings_device(h, pcm.data(), off, len, 1, sl, scores.data(), raw.data(), nullptr);
            kws_stream_batch *sb = nullptr;
            int stream_rc = (int)kws_streams_create(h, 1, &sb);
            for (int k = 0; k < 8 && !stream_rc && sl > 0; k++) {
                int produced = 0;
                stream_rc = (int)kws_streams_step_device(sb, pcm.data(), sl, nullptr, scores.data(), &produced, nullptr);
            }
            if (sl == 0) stream_rc = (int)EI_IMPULSE_DSP_ERROR;        // (a zero-length slice: the step's frame count is 0)
            kws_streams_destroy(sb);
            size_t w = 0;
            const int count_rc = (int)kws_scan_window_count(h, 40000, sl, &w);
            printf("slicing %zu %d %d %d\n", sl, scan_rc, stream_rc, count_rc);
        }
        const size_t off2[3] = { 0, 5, 7 }, len2[3] = { 15999, 100, 0 };
        printf("null %d\n", (int)kws_scan_recordings_device(h, pcm.data(), off2, len2, 3, 4000, nullptr, raw.data(), nullptr));
        printf("nullpcm %d\n", (int)kws_scan_recordings_device(h, nullptr, off2, len2, 3, 4000, scores.data(), nullptr, nullptr));
        std::fill(scores.begin(), scores.end(), -7.0f);
        rc = kws_scan_recordings_device(h, pcm.data(), nullptr, nullptr, 0, 4000, scores.data(), raw.data(), nullptr);
        bool untouched = true;
        for (float v : scores) untouched = untouched && v == -7.0f;
        printf("empty %d %d\n", (int)rc, untouched ? 1 : 0);
        rc = kws_scan_recordings_device(h, pcm.data(), off2, len2, 3, 4000, scores.data(), raw.data(), nullptr);
        for (float v : scores) untouched = untouched && v == -7.0f;
        printf("short %d %d\n", (int)rc, untouched ? 1 : 0);
        // a call that does work (host logic only): recordings at odd offsets, one of them long enough for several chunks of staged slices
        std::vector<int16_t> big(9000001, 5);
        std::vector<float> s2(3000 * C), r2(3000 * C);
        const size_t off3[4] = { 1, 17, 40001, 123 }, len3[4] = { 40000, 16319, 8000000, 24000 };
        for (int mode = 0; mode < 2; mode++) {
            if (kws_set_mode(h, mode) != EI_IMPULSE_OK) continue;
            rc = kws_scan_recordings_device(h, big.data(), off3, len3, 4, 4000, s2.data(), mode ? nullptr : r2.data(), nullptr);
            size_t nfb = 0;
            (void)kws_fast_fallback_count(h, &nfb);
            printf("full %d %d\n", mode, (int)rc);
        }
        kws_destroy(h);
    }
    return 0;
}
