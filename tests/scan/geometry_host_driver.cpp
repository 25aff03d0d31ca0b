// geometry_host_driver.cpp -- TEST INFRASTRUCTURE ONLY (tests/test_continuous_geometry.py): the window counts and slicing rules of the three
// continuous-mode APIs (stream steps, recording scan, live sessions) at any slicing, run against the stub HIP runtime of tests/sanitize
// (device memory = host heap, launches do nothing) under ASan + UBSan.  No value a kernel would write means anything here.
// usage: kws_geometry_san model.kwsm steps slice[,slice...] n_samples[,n_samples...]        prints:
//   model <path> rc <kws_create's code>
//   slicing <slice> <window-count code> <scan code> <live-create code> <stream code> <stream step> <produced>
//       stream code: the first failing step's code of a fresh S = 1 batch stepped `steps` times (0: none), stream step: that step (or
//       `steps`), produced: the steps that reported *produced before it
//   count <slice> <n_samples> <scan windows> <live windows, finished> <live windows, not finished> <live windows, pushed in two halves> <that push's code>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../include/kws/kws.h"

static std::vector<size_t> parse_list(const char *s)
{
    std::vector<size_t> v;
    for (char *end = nullptr; *s; s = *end ? end + 1 : end) {
        v.push_back((size_t)strtoull(s, &end, 10));
        if (end == s) break;
    }
    return v;
}

int main(int argc, char **argv)
{
    if (argc != 5) {
        fprintf(stderr, "usage: %s model.kwsm steps slices lengths\n", argv[0]);
        return 2;
    }
    kws_handle *h = nullptr;
    EI_IMPULSE_ERROR rc = kws_create_from_file(argv[1], 0, &h);
    printf("model %s rc %d\n", argv[1], (int)rc);
    if (rc) return 0;
    const int steps = atoi(argv[2]);
    const std::vector<size_t> slicings = parse_list(argv[3]), lengths = parse_list(argv[4]);
    const size_t C = (size_t)kws_label_count(h);
    std::vector<float> scores(4 * C, -7.0f), raw(4 * C, -7.0f);
    for (size_t sl : slicings) {
        size_t w = 0;
        const int count_rc = (int)kws_scan_window_count(h, 40 * sl, sl, &w);
        std::vector<int16_t> pcm(sl * 3 + 64, 3);
        const size_t off[1] = { 1 }, len[1] = { sl };
        const int scan_rc = (int)kws_scan_recordings_device(h, pcm.data(), off, len, 1, sl, scores.data(), raw.data(), nullptr);
        kws_live *lv = nullptr;
        const int live_rc = (int)kws_live_create(h, 2, sl, &lv);
        kws_stream_batch *sb = nullptr;
        int stream_rc = (int)kws_streams_create(h, 1, &sb), k = 0, produced_steps = 0;
        for (; k < steps && !stream_rc && sl > 0; k++) {
            int produced = 0;
            stream_rc = (int)kws_streams_step_device(sb, pcm.data(), sl, nullptr, scores.data(), &produced, nullptr);
            if (!stream_rc) produced_steps += produced;
            else break;
        }
        if (sl == 0) stream_rc = (int)EI_IMPULSE_DSP_ERROR;        // (a zero-length slice: the step's frame count is 0)
        kws_streams_destroy(sb);
        printf("slicing %zu %d %d %d %d %d %d\n", sl, count_rc, scan_rc, live_rc, stream_rc, k, produced_steps);
        if (count_rc || live_rc) {
            kws_live_destroy(lv);
            continue;
        }
        for (size_t n : lengths) {
            size_t ws = 0, wf = 0, wo = 0, wb = 0;
            (void)kws_scan_window_count(h, n, sl, &ws);
            (void)kws_live_window_count(lv, 0, n, 1, &wf);
            (void)kws_live_window_count(lv, 0, n, 0, &wo);
            // stream 1: the first half pushed (the host bookkeeping of a push; the stub launches nothing), then the rest counted with a finish
            const size_t st[1] = { 1 }, offs[1] = { 0 }, lens[1] = { n / 2 };
            size_t nw[1] = { 0 };
            std::vector<float> out((ws + 4) * C, -7.0f);
            const int push_rc = (int)kws_live_push_device(lv, 1, st, pcm.data(), offs, lens, nullptr, out.data(), nullptr, nw, nullptr);
            (void)kws_live_window_count(lv, 1, n - n / 2, 1, &wb);
            (void)kws_live_reset(lv, st, 1);
            printf("count %zu %zu %zu %zu %zu %zu %d\n", sl, n, ws, wf, wo, nw[0] + wb, push_rc);
        }
        kws_live_destroy(lv);
    }
    kws_destroy(h);
    return 0;
}
