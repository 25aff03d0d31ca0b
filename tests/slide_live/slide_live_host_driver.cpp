// slide_live_host_driver.cpp -- TEST INFRASTRUCTURE ONLY (tests/test_slide_live_host.py): the argument checks and the host arithmetic of
// kws_slide_live_*, run against the stub HIP runtime of tests/sanitize (device memory = host heap, launches do nothing) under ASan + UBSan.
// No value a kernel would write means anything here.
// usage: kws_slide_live_san model.kwsm ...   prints, per model:
//   model <path> rc <kws_create's code>
//   geom <frame stride> <clip> <frames>
//   path <hop> <flags> <create code> <kws_slide_live_path>
//   chunked <hop> <flags> <pushes> <count mismatches> <streams whose windows differ from the slide's count> <first failing push code>
//   refuse <name> <code> <state unchanged>           state unchanged: every stream's window count for a probe push is what it was before
//   big <hop> <code> <path> <samples> <windows> <the slide's count for as many samples>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <random>
#include <vector>

#include "../../include/kws/kws.h"

// each stream's window count for a probe push of 12 345 samples: changes whenever a stream's state does
static std::vector<size_t> probe(kws_slide_live *sl, size_t S)
{
    std::vector<size_t> v(S, 0);
    for (size_t s = 0; s < S; s++) (void)kws_slide_live_window_count(sl, s, 12345, &v[s]);
    return v;
}

int main(int argc, char **argv)
{
    for (int a = 1; a < argc; a++) {
        kws_handle *h = nullptr;
        EI_IMPULSE_ERROR rc = kws_create_from_file(argv[a], 0, &h);
        printf("model %s rc %d\n", argv[a], (int)rc);
        if (rc) continue;
        const size_t C = (size_t)kws_label_count(h), F = (size_t)kws_feature_count(h);
        const size_t stride = (size_t)kws_frame_stride_samples(h), clip = (size_t)kws_clip_samples(h);
        printf("geom %zu %zu %d\n", stride, clip, kws_frame_count(h));
        const size_t hops[] = { stride, 2 * stride, 4000, 48 * stride, 49 * stride, 1000, 7, clip, clip + 13 };
        const size_t S = 8;
        std::vector<int16_t> pcm(3 * clip + 64, 3);
        std::vector<float> scores(64 * C), feats(64 * F);
        for (size_t hop : hops) {
            for (int flags = 0; flags < 3; flags++) {
                kws_slide_live *sl = nullptr;
                rc = kws_slide_live_create(h, S, hop, flags, &sl);
                printf("path %zu %d %d %d\n", hop, flags, (int)rc, kws_slide_live_path(sl));
                if (rc) continue;
                // seeded random chunkings: packets of 0 samples to 3 clips to random subsets of the streams
                std::mt19937_64 rng(17 + hop * 3 + flags);
                std::vector<size_t> total(S, 0), got(S, 0);
                int pushes = 0, mismatches = 0, first_bad = 0;
                size_t diff_streams = 0;
                for (int p = 0; p < 40; p++) {
                    std::vector<size_t> st, off, len, nw;
                    for (size_t s = 0; s < S; s++) {
                        if (rng() % 3 == 0) continue;
                        const size_t kind = rng() % 4;
                        const size_t n = kind == 0 ? rng() % 4 : kind == 1 ? 1 + rng() % 400 : kind == 2 ? 1 + rng() % clip : rng() % (3 * clip + 1);
                        st.push_back(s);
                        off.push_back(rng() % 64);
                        len.push_back(n);
                    }
                    if (rng() % 2) std::reverse(st.begin(), st.end());      // entries in any order of streams
                    std::vector<size_t> want(st.size());
                    for (size_t i = 0; i < st.size(); i++) (void)kws_slide_live_window_count(sl, st[i], len[i], &want[i]);
                    size_t sum = 0;
                    for (size_t w : want) sum += w;
                    if (sum * C > scores.size()) scores.resize(sum * C);
                    if (sum * F > feats.size()) feats.resize(sum * F);
                    nw.assign(st.size(), 7777);
                    rc = kws_slide_live_push_device(sl, st.size(), st.data(), pcm.data(), off.data(), len.data(), scores.data(), p % 2 ? feats.data() : nullptr,
                                                    nw.data(), nullptr);
                    pushes++;
                    if (rc && !first_bad) first_bad = (int)rc;
                    for (size_t i = 0; i < st.size(); i++) {
                        mismatches += nw[i] != want[i];
                        total[st[i]] += len[i];
                        got[st[i]] += nw[i];
                    }
                    if (p % 10 == 9) {
                        for (size_t s = 0; s < S; s++) {
                            size_t w = 0;
                            (void)kws_slide_window_count(h, total[s], hop, &w);
                            diff_streams += w != got[s];
                        }
                        // reset streams start over: their counts so far are dropped
                        const size_t rs[2] = { 1, 5 };
                        if (kws_slide_live_reset(sl, p == 19 ? nullptr : rs, p == 19 ? 0 : 2) == EI_IMPULSE_OK) {
                            if (p == 19) for (size_t s = 0; s < S; s++) total[s] = got[s] = 0;
                            else for (size_t s : rs) total[s] = got[s] = 0;
                        }
                    }
                }
                printf("chunked %zu %d %d %d %zu %d\n", hop, flags, pushes, mismatches, diff_streams, first_bad);
                kws_slide_live_destroy(sl);
            }
        }
        // refusals change no state
        {
            struct Case { const char *name; int rc; };
            std::vector<Case> cases;
            kws_slide_live *bad = nullptr;
            cases.push_back({ "create_s0", (int)kws_slide_live_create(h, 0, stride, 0, &bad) });
            cases.push_back({ "create_sbig", (int)kws_slide_live_create(h, (size_t)1 << 30, stride, 0, &bad) });
            cases.push_back({ "create_hop0", (int)kws_slide_live_create(h, S, 0, 0, &bad) });
            cases.push_back({ "create_hopbig", (int)kws_slide_live_create(h, S, ((size_t)1 << 56) + 1, 0, &bad) });
            cases.push_back({ "create_flags", (int)kws_slide_live_create(h, S, stride, 3, &bad) });
            cases.push_back({ "create_flagsneg", (int)kws_slide_live_create(h, S, stride, -1, &bad) });
            cases.push_back({ "create_shared7", (int)kws_slide_live_create(h, S, 7, KWS_SLIDE_SHARED, &bad) });
            cases.push_back({ "create_shared49", (int)kws_slide_live_create(h, S, 49 * stride, KWS_SLIDE_SHARED, &bad) });
            cases.push_back({ "create_nullout", (int)kws_slide_live_create(h, S, stride, 0, nullptr) });
            cases.push_back({ "create_nullhandle", (int)kws_slide_live_create(nullptr, S, stride, 0, &bad) });
            if (bad) cases.push_back({ "create_left_a_session", 0 });
            kws_slide_live *sl = nullptr;
            rc = kws_slide_live_create(h, S, stride, 0, &sl);
            if (rc) { printf("create %d\n", (int)rc); kws_destroy(h); continue; }
            const size_t half[2] = { 2, 3 };
            const size_t o2[2] = { 0, 0 }, l2[2] = { clip + 9000, 17 };
            size_t n2[2] = { 0, 0 };
            (void)kws_slide_live_push_device(sl, 2, half, pcm.data(), o2, l2, scores.data(), nullptr, n2, nullptr);
            const std::vector<size_t> before = probe(sl, S);
            const size_t dup[2] = { 4, 4 }, out_of_range[2] = { 1, S }, lmany[2] = { 17, ((size_t)1 << 60) };
            cases.push_back({ "duplicate", (int)kws_slide_live_push_device(sl, 2, dup, pcm.data(), o2, l2, scores.data(), nullptr, n2, nullptr) });
            cases.push_back({ "range", (int)kws_slide_live_push_device(sl, 2, out_of_range, pcm.data(), o2, l2, scores.data(), nullptr, n2, nullptr) });
            cases.push_back({ "nullstreams", (int)kws_slide_live_push_device(sl, 2, nullptr, pcm.data(), o2, l2, scores.data(), nullptr, n2, nullptr) });
            cases.push_back({ "nulllengths", (int)kws_slide_live_push_device(sl, 2, half, pcm.data(), o2, nullptr, scores.data(), nullptr, n2, nullptr) });
            cases.push_back({ "nullcounts", (int)kws_slide_live_push_device(sl, 2, half, pcm.data(), o2, l2, scores.data(), nullptr, nullptr, nullptr) });
            cases.push_back({ "nullscores", (int)kws_slide_live_push_device(sl, 2, half, pcm.data(), o2, l2, nullptr, nullptr, n2, nullptr) });
            cases.push_back({ "nullpcm", (int)kws_slide_live_push_device(sl, 2, half, nullptr, o2, l2, scores.data(), nullptr, n2, nullptr) });
            cases.push_back({ "nulloffsets", (int)kws_slide_live_push_device(sl, 2, half, pcm.data(), nullptr, l2, scores.data(), nullptr, n2, nullptr) });
            cases.push_back({ "nullsession", (int)kws_slide_live_push_device(nullptr, 2, half, pcm.data(), o2, l2, scores.data(), nullptr, n2, nullptr) });
            cases.push_back({ "toomany", (int)kws_slide_live_push_device(sl, 2, half, pcm.data(), o2, lmany, scores.data(), nullptr, n2, nullptr) });
            cases.push_back({ "resetrange", (int)kws_slide_live_reset(sl, out_of_range, 2) });
            cases.push_back({ "resetnull", (int)kws_slide_live_reset(sl, nullptr, 2) });
            size_t w = 0;
            cases.push_back({ "countrange", (int)kws_slide_live_window_count(sl, S, 10, &w) });
            cases.push_back({ "countnull", (int)kws_slide_live_window_count(sl, 0, 10, nullptr) });
            cases.push_back({ "countmany", (int)kws_slide_live_window_count(sl, 2, (size_t)1 << 60, &w) });
            const bool same = probe(sl, S) == before && n2[0] == 1 + 9000 / stride && n2[1] == 0;
            for (const Case &c : cases) printf("refuse %s %d %d\n", c.name, c.rc, same ? 1 : 0);
            // zero-length pushes need no pcm / offsets; an empty push needs nothing
            const size_t l0[2] = { 0, 0 };
            printf("refuse zerolen %d %d\n", (int)kws_slide_live_push_device(sl, 2, half, nullptr, nullptr, l0, scores.data(), nullptr, n2, nullptr),
                   probe(sl, S) == before ? 1 : 0);
            printf("refuse empty %d %d\n", (int)kws_slide_live_push_device(sl, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr),
                   probe(sl, S) == before ? 1 : 0);
            kws_slide_live_destroy(sl);
        }
        // one stream pushed past 2^32 samples in large packets (host bookkeeping only), on both paths
        std::vector<int16_t> big(3000001, 5);
        const size_t big_hops[2] = { stride, 4000 };
        for (size_t hop : big_hops) {
            kws_slide_live *lb = nullptr;
            rc = kws_slide_live_create(h, 3, hop, 0, &lb);
            size_t total = 0, total_w = 0, want_w = 0;
            std::vector<float> s2;
            for (int p = 0; p < 1440 && !rc; p++) {
                const size_t st[1] = { 1 }, off[1] = { (size_t)(p & 1) }, len[1] = { 3000000 - (size_t)(p % 7) };
                size_t nw[1] = { 0 }, want = 0;
                (void)kws_slide_live_window_count(lb, 1, len[0], &want);
                if (s2.size() < want * C + 1) s2.resize(want * C + 1);
                rc = kws_slide_live_push_device(lb, 1, st, big.data(), off, len, s2.data(), nullptr, nw, nullptr);
                if (!rc && nw[0] != want) rc = (EI_IMPULSE_ERROR)-1;
                total += len[0];
                total_w += nw[0];
            }
            (void)kws_slide_window_count(h, total, hop, &want_w);
            printf("big %zu %d %d %zu %zu %zu\n", hop, (int)rc, kws_slide_live_path(lb), total, total_w, want_w);
            kws_slide_live_destroy(lb);
        }
        kws_destroy(h);
    }
    return 0;
}
