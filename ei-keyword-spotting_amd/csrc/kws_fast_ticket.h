// kws_fast_ticket.h -- how the three-waves-per-SIMD fast kernel maps tickets to clips (kws_fast.hip: the clip loop; DESIGN.md 4.4 "Clips by ticket").
// Host and device compile the same lines (tests/fast_ticket/fast_ticket_driver.cpp, run by tests/test_fast_ticket_host.py, deals whole launches out
// without a GPU).
//
// A wave's first clip is its own number in the grid; clips [stride, n_sel) -- stride = the grid's wave count -- are dealt out by tickets.  One head word
// for the whole grid is one address that every wave's returning add meets at: 2 816 waves draw at launch start, ~60 draws per microsecond arrive in steady state,
// and one word serves ~88.  So the clips behind the first stride are dealt round-robin onto KWS_FAST_TICKET_SHARDS heads, each on a 128-byte line of its own:
//     ticket t of shard s  <->  clip stride + SHARDS t + s
// A workgroup draws from its home shard (block index modulo SHARDS: the blocks of one XCD share a head).  A wave whose home ticket lies past the last clip
// walks the other shards in order, one draw each, and leaves when all of them are past the end -- a head that has handed out one ticket past the end has
// handed out every ticket in front of it, so nothing is left behind.  The word that counts the waves that have left sits on a line of its own behind the heads.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define KWS_TICKET_HD __host__ __device__
#else
#define KWS_TICKET_HD
#endif

#ifndef KWS_FAST_TICKET_SHARDS
#define KWS_FAST_TICKET_SHARDS 8
#endif
#define KWS_FAST_TICKET_LINE 32                                                          // ints per 128-byte line
#define KWS_FAST_TICKET_WORDS ((KWS_FAST_TICKET_SHARDS + 1) * KWS_FAST_TICKET_LINE)      // the block in device memory, zero between launches

KWS_TICKET_HD static inline int kws_fast_ticket_home(int block) { return block % KWS_FAST_TICKET_SHARDS; }
KWS_TICKET_HD static inline int kws_fast_ticket_head(int shard) { return shard * KWS_FAST_TICKET_LINE; }              // word index of a shard's head
KWS_TICKET_HD static inline int kws_fast_ticket_gone(void) { return KWS_FAST_TICKET_SHARDS * KWS_FAST_TICKET_LINE; }  // word index of the leavers' count
KWS_TICKET_HD static inline int kws_fast_ticket_clip(int stride, int shard, int t) { return stride + KWS_FAST_TICKET_SHARDS * t + shard; }

// The walk of a wave whose home shard is exhausted.  draw(s) returns the value a returning add of 1 on shard s's head gave (waited for on the spot).
// Returns the clip it found, or a value >= n_sel when every shard is past the end.
template <class Draw>
KWS_TICKET_HD static inline int kws_fast_ticket_walk(int stride, int n_sel, int home, Draw draw)
{
    int c = n_sel;
#pragma unroll 1
    for (int k = 1; k < KWS_FAST_TICKET_SHARDS; ++k) {
        const int s = home + k < KWS_FAST_TICKET_SHARDS ? home + k : home + k - KWS_FAST_TICKET_SHARDS;
        c = kws_fast_ticket_clip(stride, s, draw(s));
        if (c < n_sel) break;
    }
    return c;
}
