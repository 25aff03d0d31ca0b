// Host driver of tests/test_fast_ticket_host.py: deals whole launches of the three-waves-per-SIMD fast kernel out on the CPU, with csrc/kws_fast_ticket.h's own
// mapping (the lines the kernel compiles), in seeded random interleavings of the waves' steps.
//
// A wave is the kernel's clip loop as a state machine -- one step per access to the ticket block, which is where waves interleave:
//     its first clip is its own number; per clip it draws from its home head, takes the clip, reads the draw as the next clip; a draw past the last clip sends
//     it round the other heads, one draw per step, until one gives a clip or all are past the end; then it counts itself out, and the last wave out zeroes
//     every head and the count.
// mode "steps": the walk round the other heads is written out here, a step per draw, so that any two walks interleave draw by draw.
// mode "walk":  the walk is kws_fast_ticket_walk itself; in front of each of its draws a random number of steps of OTHER waves run (waves that are inside a
//               walk of their own further up the stack wait, as a wave that waits for its draw does).
//
// usage: fast_ticket_driver <mode> <seed> <stride> <waves per workgroup> <n_sel from> <n_sel to>
// prints one line per failing case and "CASES <n> FAIL <m>" at the end.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "kws_fast_ticket.h"

static uint64_t rng_state;
static uint32_t rnd()
{
    rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(rng_state >> 33);
}

enum { DRAW_HOME, TAKE, WALK, LEAVE, GONE };

struct Wave {
    int state, ci, ni, tv, home, k;
    bool busy;                                    // inside kws_fast_ticket_walk further up the stack
};

struct Launch {
    int stride, wpw, n_sel;
    bool use_walk;
    std::vector<int> words;                       // the ticket block: heads + the leavers' count
    std::vector<int> taken;
    std::vector<Wave> w;
    std::vector<int> live;                        // indices of the waves that have not left
    long steps = 0;
    int errors = 0, depth = 0;

    int add(int word) { return words.at((size_t)word)++; }

    void leave(Wave &v)
    {
        const int gone = add(kws_fast_ticket_gone());
        if (gone == stride - 1) {
            for (int s = 0; s < KWS_FAST_TICKET_SHARDS; ++s) words.at((size_t)kws_fast_ticket_head(s)) = 0;
            words.at((size_t)kws_fast_ticket_gone()) = 0;
        }
        v.state = GONE;
    }

    void others(int n)
    {
        if (depth >= 48) return;                  // (walks nested inside walks: bounded, so that the stack is)
        ++depth;
        for (int i = 0; i < n && !live.empty(); ++i) {
            const size_t at = rnd() % live.size();
            if (!w[(size_t)live[at]].busy) step(at);
        }
        --depth;
    }

    // one step of wave live[at]; removes it from `live` when it has left
    void step(size_t at)
    {
        const int id = live[at];
        Wave &v = w[(size_t)id];
        ++steps;
        switch (v.state) {
        case DRAW_HOME:
            if (v.ci >= n_sel) { v.state = LEAVE; break; }
            v.tv = add(kws_fast_ticket_head(v.home));
            v.state = TAKE;
            break;
        case TAKE:
            if (v.ci < 0 || v.ci >= n_sel) { ++errors; v.state = LEAVE; break; }
            ++taken[(size_t)v.ci];
            v.ni = kws_fast_ticket_clip(stride, v.home, v.tv);
            if (v.ni < n_sel) { v.ci = v.ni; v.state = DRAW_HOME; break; }
            if (use_walk) {
                v.busy = true;
                v.ni = kws_fast_ticket_walk(stride, n_sel, v.home, [&](int s) {
                    others((int)(rnd() % 7));
                    return add(kws_fast_ticket_head(s));
                });
                w[(size_t)id].busy = false;
                w[(size_t)id].ci = w[(size_t)id].ni;
                w[(size_t)id].state = DRAW_HOME;
                return;                                            // (`live` may have changed under the walk: this wave is looked up again by its next step)
            }
            v.k = 1;
            v.state = KWS_FAST_TICKET_SHARDS > 1 ? WALK : DRAW_HOME;
            v.ci = v.ni;
            break;
        case WALK: {
            const int s = (v.home + v.k) % KWS_FAST_TICKET_SHARDS;
            v.ni = kws_fast_ticket_clip(stride, s, add(kws_fast_ticket_head(s)));
            ++v.k;
            if (v.ni < n_sel || v.k >= KWS_FAST_TICKET_SHARDS) { v.ci = v.ni; v.state = DRAW_HOME; }
            break;
        }
        case LEAVE:
            leave(v);
            break;
        }
        if (w[(size_t)id].state == GONE) {
            // (the walk's nested steps may have moved the wave inside `live`)
            for (size_t i = 0; i < live.size(); ++i)
                if (live[i] == id) { live[i] = live.back(); live.pop_back(); break; }
        }
    }

    bool run()
    {
        words.assign((size_t)KWS_FAST_TICKET_WORDS, 0);
        taken.assign((size_t)(n_sel > 0 ? n_sel : 0), 0);
        w.assign((size_t)stride, Wave());
        live.clear();
        for (int i = 0; i < stride; ++i) {
            w[(size_t)i] = Wave{ DRAW_HOME, i, 0, 0, kws_fast_ticket_home(i / wpw), 0, false };
            live.push_back(i);
        }
        // every wave ends: a wave makes at most one step per ticket block access, and the accesses of a launch are bounded
        const long limit = 64L * (n_sel + stride) * (KWS_FAST_TICKET_SHARDS + 4) + 1024;
        while (!live.empty() && steps < limit) step(rnd() % live.size());
        bool ok = live.empty() && errors == 0;
        for (int c = 0; c < n_sel; ++c) ok = ok && taken[(size_t)c] == 1;
        for (int x : words) ok = ok && x == 0;
        return ok;
    }
};

int main(int argc, char **argv)
{
    if (argc < 7) { fprintf(stderr, "usage: %s steps|walk seed stride waves_per_workgroup n_sel_from n_sel_to\n", argv[0]); return 2; }
    const bool use_walk = strcmp(argv[1], "walk") == 0;
    rng_state = strtoull(argv[2], nullptr, 10) * 2654435761ull + 12345;
    const int stride = atoi(argv[3]), wpw = atoi(argv[4]), from = atoi(argv[5]), to = atoi(argv[6]);
    if (stride < 1 || wpw < 1 || stride % wpw != 0) { fprintf(stderr, "stride must be a multiple of the waves per workgroup\n"); return 2; }
    // the layout: a head per 128-byte line, the count on a line of its own behind them
    int bad = 0, n = 0;
    for (int s = 0; s < KWS_FAST_TICKET_SHARDS; ++s)
        if (kws_fast_ticket_head(s) * 4 != 128 * s) ++bad;
    if (kws_fast_ticket_gone() * 4 != 128 * KWS_FAST_TICKET_SHARDS || KWS_FAST_TICKET_WORDS * 4 != 128 * (KWS_FAST_TICKET_SHARDS + 1)) ++bad;
    if (bad) printf("LAYOUT\n");
    for (int n_sel = from; n_sel <= to; ++n_sel) {
        Launch L;
        L.stride = stride; L.wpw = wpw; L.n_sel = n_sel; L.use_walk = use_walk;
        ++n;
        if (!L.run()) {
            ++bad;
            printf("FAILED stride %d n_sel %d: %zu waves still running, %d errors\n", stride, n_sel, L.live.size(), L.errors);
        }
    }
    printf("CASES %d FAIL %d\n", n, bad);
    return 0;
}
