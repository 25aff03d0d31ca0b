// live_host_driver.cpp -- TEST INFRASTRUCTURE ONLY (tests/test_live_host.py): the argument checks and the host arithmetic of kws_live_*,
// run against the stub HIP runtime of tests/sanitize (device memory = host heap, launches do nothing) under ASan + UBSan.  No value a kernel
// would write means anything here.
// usage: kws_live_san model.kwsm ...   prints, per model:
//   model <path> rc <kws_create's code>
//   slicing <slice> <create code> <scan window-count code>
//   create0 <code>                                   S = 0
//   chunked <pushes> <count mismatches> <streams whose windows differ from the scan's count> <first failing push code>
//   refuse <name> <code> <state unchanged>           state unchanged: every stream's window count for a probe push is what it was before
//   big <mode> <code> <windows>                      pushes long enough for several chunks of staged slices
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <random>
#include <vector>

#include "../../include/kws/kws.h"

static const size_t kSlice = 4000;

// each stream's window count for a probe push of 12 345 samples, finishing: changes whenever a stream's state does
static std::vector<size_t> probe(kws_live *lv, size_t S)
{
    std::vector<size_t> v(S, 0);
    for (size_t s = 0; s < S; s++) (void)kws_live_window_count(lv, s, 12345, 1, &v[s]);
    return v;
}

int main(int argc, char **argv)
{
    for (int a = 1; a < argc; a++) {
        kws_handle *h = nullptr;
        EI_IMPULSE_ERROR rc = kws_create_from_file(argv[a], 0, &h);
        printf("model %s rc %d\n", argv[a], (int)rc);
        if (rc) continue;
        const size_t C = (size_t)kws_label_count(h);
        const size_t slicings[] = { 4000, 4001, 100, 0, 8000, 16000, 3200 };
        for (size_t sl : slicings) {
            kws_live *lv = nullptr;
            const int create_rc = (int)kws_live_create(h, 2, sl, &lv);
            size_t w = 0;
            const int count_rc = (int)kws_scan_window_count(h, 40000, sl, &w);
            printf("slicing %zu %d %d\n", sl, create_rc, count_rc);
            kws_live_destroy(lv);
        }
        {
            kws_live *lv = nullptr;
            printf("create0 %d\n", (int)kws_live_create(h, 0, kSlice, &lv));
        }
        // seeded random chunkings: packets of 1 sample to 3 s to random subsets of 8 streams, then every stream finished
        const size_t S = 8;
        std::vector<int16_t> pcm(3 * 16000 + 64, 3);
        std::vector<float> scores(64 * C), raw(64 * C);
        kws_live *lv = nullptr;
        rc = kws_live_create(h, S, kSlice, &lv);
        if (rc) { printf("create %d\n", (int)rc); kws_destroy(h); continue; }
        std::mt19937_64 rng(17);
        std::vector<size_t> total(S, 0), got(S, 0);
        int pushes = 0, mismatches = 0, first_bad = 0;
        size_t diff_streams = 0;
        for (int round = 0; round < 3; round++) {
            for (int p = 0; p < 120; p++) {
                std::vector<size_t> st, off, len, nw;
                std::vector<int> fin;
                for (size_t s = 0; s < S; s++) {
                    if (rng() % 3 == 0) continue;
                    const size_t kind = rng() % 4;
                    const size_t n = kind == 0 ? rng() % 4 : kind == 1 ? 1 + rng() % 400 : kind == 2 ? 1 + rng() % 8000 : 1 + rng() % 48000;
                    st.push_back(s);
                    off.push_back(rng() % 64);
                    len.push_back(n);
                    fin.push_back(p == 119 || rng() % 97 == 0);
                }
                if (rng() % 2) std::reverse(st.begin(), st.end());      // entries in any order of streams
                std::vector<size_t> want(st.size());
                for (size_t i = 0; i < st.size(); i++) (void)kws_live_window_count(lv, st[i], len[i], fin[i], &want[i]);
                size_t sum = 0;
                for (size_t w : want) sum += w;
                if (sum * C > scores.size()) { scores.resize(sum * C); raw.resize(sum * C); }
                nw.assign(st.size(), 7777);
                rc = kws_live_push_device(lv, st.size(), st.data(), pcm.data(), off.data(), len.data(), fin.data(), scores.data(), raw.data(), nw.data(), nullptr);
                pushes++;
                if (rc && !first_bad) first_bad = (int)rc;
                for (size_t i = 0; i < st.size(); i++) {
                    mismatches += nw[i] != want[i];
                    total[st[i]] += len[i];
                    got[st[i]] += nw[i];
                    if (fin[i]) {
                        size_t w = 0;
                        (void)kws_scan_window_count(h, total[st[i]], kSlice, &w);
                        diff_streams += w != got[st[i]];
                        total[st[i]] = got[st[i]] = 0;
                    }
                }
            }
            if (round == 1) {
                // a reset stream starts over: its count so far is dropped
                const size_t rs[2] = { 1, 5 };
                if (kws_live_reset(lv, rs, 2) == EI_IMPULSE_OK) for (size_t s : rs) total[s] = got[s] = 0;
            }
        }
        printf("chunked %d %d %zu %d\n", pushes, mismatches, diff_streams, first_bad);
        // refusals change no state
        {
            const size_t half[2] = { 2, 3 };
            const size_t o2[2] = { 0, 0 }, l2[2] = { 9000, 17 };
            size_t n2[2] = { 0, 0 };
            (void)kws_live_push_device(lv, 2, half, pcm.data(), o2, l2, nullptr, scores.data(), nullptr, n2, nullptr);
            const std::vector<size_t> before = probe(lv, S);
            struct Case { const char *name; int rc; };
            std::vector<Case> cases;
            const size_t dup[2] = { 4, 4 }, out_of_range[2] = { 1, S };
            cases.push_back({ "duplicate", (int)kws_live_push_device(lv, 2, dup, pcm.data(), o2, l2, nullptr, scores.data(), nullptr, n2, nullptr) });
            cases.push_back({ "range", (int)kws_live_push_device(lv, 2, out_of_range, pcm.data(), o2, l2, nullptr, scores.data(), nullptr, n2, nullptr) });
            cases.push_back({ "nullstreams", (int)kws_live_push_device(lv, 2, nullptr, pcm.data(), o2, l2, nullptr, scores.data(), nullptr, n2, nullptr) });
            cases.push_back({ "nulllengths", (int)kws_live_push_device(lv, 2, half, pcm.data(), o2, nullptr, nullptr, scores.data(), nullptr, n2, nullptr) });
            cases.push_back({ "nullcounts", (int)kws_live_push_device(lv, 2, half, pcm.data(), o2, l2, nullptr, scores.data(), nullptr, nullptr, nullptr) });
            cases.push_back({ "nullscores", (int)kws_live_push_device(lv, 2, half, pcm.data(), o2, l2, nullptr, nullptr, nullptr, n2, nullptr) });
            cases.push_back({ "nullpcm", (int)kws_live_push_device(lv, 2, half, nullptr, o2, l2, nullptr, scores.data(), nullptr, n2, nullptr) });
            cases.push_back({ "nulloffsets", (int)kws_live_push_device(lv, 2, half, pcm.data(), nullptr, l2, nullptr, scores.data(), nullptr, n2, nullptr) });
            cases.push_back({ "nullsession", (int)kws_live_push_device(nullptr, 2, half, pcm.data(), o2, l2, nullptr, scores.data(), nullptr, n2, nullptr) });
            cases.push_back({ "resetrange", (int)kws_live_reset(lv, out_of_range, 2) });
            cases.push_back({ "resetnull", (int)kws_live_reset(lv, nullptr, 2) });
            size_t w = 0;
            cases.push_back({ "countrange", (int)kws_live_window_count(lv, S, 10, 0, &w) });
            cases.push_back({ "countnull", (int)kws_live_window_count(lv, 0, 10, 0, nullptr) });
            const bool same = probe(lv, S) == before;
            for (const Case &c : cases) printf("refuse %s %d %d\n", c.name, c.rc, same ? 1 : 0);
            // zero-length pushes without samples need no pcm / offsets; an empty push needs nothing
            const size_t l0[2] = { 0, 0 };
            printf("refuse zerolen %d %d\n", (int)kws_live_push_device(lv, 2, half, nullptr, nullptr, l0, nullptr, scores.data(), nullptr, n2, nullptr),
                   probe(lv, S) == before ? 1 : 0);
            printf("refuse empty %d %d\n", (int)kws_live_push_device(lv, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr),
                   probe(lv, S) == before ? 1 : 0);
        }
        kws_live_destroy(lv);
        // pushes long enough for several chunks of staged slices (host bookkeeping only), in both modes
        std::vector<int16_t> big(3000001, 5);
        for (int mode = 0; mode < 2; mode++) {
            if (kws_set_mode(h, mode) != EI_IMPULSE_OK) continue;
            kws_live *lb = nullptr;
            rc = kws_live_create(h, 8, kSlice, &lb);
            size_t total_w = 0;
            for (int p = 0; p < 3 && !rc; p++) {
                const size_t st[8] = { 0, 1, 2, 3, 4, 5, 6, 7 };
                const size_t off[8] = { 1, 17, 3, 0, 5, 7, 9, 11 };
                const size_t len[8] = { 2999000, 2999001, 2999999, 2999990, 1000, 2500000, 2999000, 2999000 };
                const int fin[8] = { p == 2, 0, 0, 0, p == 2, 0, p == 2, 0 };
                size_t nw[8];
                size_t want = 0;
                for (int i = 0; i < 8; i++) { size_t w = 0; (void)kws_live_window_count(lb, st[i], len[i], fin[i], &w); want += w; }
                std::vector<float> s2(want * C + 1), r2(want * C + 1);
                rc = kws_live_push_device(lb, 8, st, big.data(), off, len, fin, s2.data(), mode ? nullptr : r2.data(), nw, nullptr);
                for (int i = 0; i < 8; i++) total_w += nw[i];
                size_t nfb = 0;
                (void)kws_fast_fallback_count(h, &nfb);
            }
            printf("big %d %d %zu\n", mode, (int)rc, total_w);
            kws_live_destroy(lb);
        }
        (void)kws_set_mode(h, KWS_MODE_EXACT);
        kws_destroy(h);
    }
    return 0;
}
