// kws_pool.h -- what the pool's units share (internal to libkws_mi355x.so): kws_pool.cpp and kws_pool_kernels.hip.  A pool is the bank's
// narrow sibling (contract in include/kws/kws.h): up to KWS_POOL_MAX int8 members of the two-block matrix-core shape behind one DSP block,
// ONE member per row, one score matrix [rows][stride].  Nothing per member travels in the launch arguments: the members' records, the work
// items and the row lists are all in HBM.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kws_bank.h"

#ifndef KWS_POOL_MAX
#define KWS_POOL_MAX 4096          // members of a pool (include/kws/kws.h)
#define KWS_POOL_NONE 0xffffffffu  // a row or stream that names no member
#endif
// Rows of one work item at most: what one workgroup runs behind one staging of its member's tables (12 KB of ADD tables and the head).
// Fewer rows per item pay the staging more often; more leave a member that holds most of a small batch on too few workgroups.  Chosen
// among 4, 8, 16, 32 and 64 (profiles/pool_rate.md): at 65 536 clips 16 is within 1.3 % of the best (64) where 4 is 6 % behind, and at
// 4 096 clips of one tenant it is within 4 % of the best (8) where 64 is 30 % behind; the live push does not feel it.
#define KWS_POOL_ITEM_ROWS 16

// One work item = one workgroup: `count` rows of member `member`, the positions first .. first + count - 1 of the call's packed row list
// (every named member's rows ascending, member after member).  Uniform over the workgroup: it is read with scalar loads.
struct KwsPoolItem {
    int member, first, count, pad;
};

// The plan predicate behind kws_nn_uses_mfma without the kws_force_scalar_nn test switch: the graph is of the two-block matrix-core shape.
int kws_pool_nn_fits(const KwsNnPlan &N);
// One launch for every item of a call, all members having activation rows of cp bytes (16 or 64).  rows [i]: a row of features [..][F]; its
// scores go to scores + row * stride.
int kws_launch_pool_nn_mfma(const KwsBankRec *recs, const KwsPoolItem *items, int n_items, const int *rows, int cp, const float *features, float *scores, int stride,
                            hipStream_t stream);
// The moving average of a live pool push: one thread per (entry, column < stride); assign [S] (a member, or KWS_POOL_NONE) and labels [K]
// in HBM; raw and scores [windows][stride]; maf [S][stride][taps + 1].
int kws_launch_pool_maf_live(const float *raw, float *scores, const long long *meta, int n_act, int stride, const uint32_t *assign, const int *labels, int k_full,
                             float *maf, hipStream_t stream);
// The moving average of a pool scan: one thread per (recording with windows, column < stride), a fresh filter each; member [n_rec] (a
// member, or KWS_POOL_NONE: the recordings that have windows, in the order of wbase [n_rec + 1]) and labels [K] in HBM; raw and scores
// [windows][stride], which may be the same buffer.
int kws_launch_pool_maf_scan(const float *raw, float *scores, const long long *wbase, int n_rec, int stride, const uint32_t *member, const int *labels,
                             hipStream_t stream);

// ---- host side (kws_pool.cpp: includes kws_internal.h first) ----------------------------------------------------------------------------------
#ifdef KWS_INTERNAL
#include <memory>

struct kws_pool {
    std::vector<kws_handle *> m;           // members, in the caller's order; calls go through m[0]'s front end and scratch
    int device = 0;
    int cp = 0;                            // bytes of an activation row of block 0: every member's (they share the feature matrix's columns)
    size_t stride = 0;                     // columns of a score row: the most labels any member has
    size_t most = 0;                       // the first member that has them (the slide's bound on windows x labels is its plan's)
    KwsBankRec *d_rec = nullptr;           // [K]
    int *d_labels = nullptr;               // [K]
    float *feat = nullptr;                 // the shared feature matrix of calls without `features`
    size_t feat_cap = 0;
    hipEvent_t ev = nullptr;               // end of the last call's work
    bool ev_used = false;
    BankUpload<int> table;                 // a call's items, then its row list: one chunk's at a time
    BankUpload<uint32_t> scan_members;     // a scan's members, one per recording that has windows (the table's host copy is the last chunk's items)
    std::vector<int> fill;                 // [K] scratch of the list builder
    std::mutex mu;
};

// member [n] (a member < K, or KWS_POOL_NONE) -> out: the items (4 ints each: member, first, count, 0), members ascending, each member's list
// cut every item_rows rows; then the packed row list.  One counting pass, one filling pass: every list is ascending.  Returns the item count;
// the rows start at out[4 * items].  fill: scratch.
KWS_INTERNAL size_t kws_pool_items(const uint32_t *member, size_t n, size_t K, int item_rows, std::vector<int> &out, std::vector<int> &fill);
// the first of n entries that is neither a member < K nor KWS_POOL_NONE: its index, or n
KWS_INTERNAL size_t kws_pool_member_check(const uint32_t *member, size_t n, size_t K);
// The per-window member table of a call, as kws_bank_window_routes builds the routes: entry i has n_windows[i] windows of member
// assign[index[i]] (a live push: the session's members by stream), or assign[i] where index is NULL (a recording call: the call's members
// by recording).
KWS_INTERNAL void kws_pool_window_members(const uint32_t *assign, const size_t *index, const size_t *n_windows, size_t n, std::vector<uint32_t> &out);
// Every named member's network from the feature matrix feat [n][F] (device): row i's scores go to scores + (row0 + i) * stride.
KWS_INTERNAL EI_IMPULSE_ERROR pool_networks(kws_pool *p, const float *feat, size_t n, const uint32_t *member, float *scores, size_t row0, hipStream_t s);
#endif
