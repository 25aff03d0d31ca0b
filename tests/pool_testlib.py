"""What the pool's tests share (tests/test_gpu_pool.py, tests/test_pool_host.py): the tenants -- synthetic int8 graphs of the stock two-block
shape, one seed each, label counts cycling through 3, 4 and 6 so that the score stride exceeds most members' labels, at both activation-row
widths of the matrix-core kernels --, the member patterns of the cases, the list and work-item builder of csrc/kws_pool.cpp restated, and
the comparer of a score matrix that was filled with a sentinel before the call.  Pure host arithmetic apart from load_tenants."""
import os

import numpy as np

from kws_testlib import bits, synth_model_blob

POOL_NONE = 0xffffffff
POOL_MAX = 4096
SENTINEL_BITS = 0x7fc0dead     # a quiet NaN no kernel here produces
KWS_NN_WAVES = 4               # rows a workgroup of the matrix-core network kernels has in flight (csrc/kws_nn_int8_dev.h)
LABELS = (3, 4, 6)
# activation rows of block 0: 16 bytes at 13 cepstral columns, 64 at 40 (kws_nn_mfma_kernel<16> / <64>)
# (49x40: the DSP block of models/cfg2_mfcc40_*.kwsm and cfg5_dscnn_mfcc40_*.kwsm, so that those files differ from a tenant in the graph alone)
WIDTHS = {"49x13": dict(ncep=13, num_filters=32), "49x40": dict(ncep=40, num_filters=40, low=300, high=0)}
PATTERNS = ("one", "robin", "heavy", "none", "never", "edges")


def tenant_kw(width, k):
    """synth_model_blob arguments of tenant k at a width: seeds distinct over both widths"""
    return dict(seed=4200 + 1000 * list(WIDTHS).index(width) + k, n_labels=LABELS[k % len(LABELS)], logit_std=1.5, **WIDTHS[width])


def write_tenants(directory, width, K):
    """the .kwsm files of tenants 0 .. K - 1 at a width, written once; their paths"""
    paths = []
    for k in range(K):
        p = os.path.join(str(directory), "tenant_%s_%03d.kwsm" % (width, k))
        if not os.path.exists(p):
            with open(p, "wb") as f:
                f.write(synth_model_blob(**tenant_kw(width, k)))
        paths.append(p)
    return paths


def load_tenants(pkg, paths):
    """the tenants as loaded models; every one must run on the matrix-core kernel, otherwise no pool test says anything"""
    models = [pkg.Model(p) for p in paths]
    for p, gm in zip(paths, models):
        assert gm.nn_kernel == "kws_nn_mfma_kernel" and not gm.is_float, (p, gm.nn_kernel)
    return models


def pattern(kind, B, K, item_rows, seed=0):
    """the member of each of B rows (uint32, POOL_NONE: nobody), or None where B or K is too small for the kind to be what it says
      one    every row names the last member
      robin  row i names member i mod K
      heavy  member 0 takes all but K - 1 rows, every other member one
      none   robin with every third row naming nobody (B = 1: that row names nobody)
      never  robin over the members but 1 mod K, whom nobody names (K = 1: every row names nobody)
      edges  in a seeded shuffle of the rows: member 0 has exactly item_rows rows, member 1 item_rows + 1 (a list of two items), member 2
             fewer than KWS_NN_WAVES, the remaining rows name nobody (K < 3: member 0 alone, with item_rows + 1 rows)"""
    i = np.arange(B)
    if kind == "one":
        return np.full(B, K - 1, np.uint32)
    if kind == "robin":
        return (i % K).astype(np.uint32)
    if kind == "heavy":
        if K < 2 or B < 2 * K:
            return None
        m = np.zeros(B, np.uint32)
        m[np.arange(1, K) * (B // K)] = np.arange(1, K)
        return m
    if kind == "none":
        m = (i % K).astype(np.uint32)
        m[::3] = POOL_NONE
        return m
    if kind == "never":
        if K == 1:
            return np.full(B, POOL_NONE, np.uint32)
        others = np.array([k for k in range(K) if k != 1 % K], np.uint32)
        return others[i % others.size]
    if kind == "edges":
        counts = [item_rows, item_rows + 1, KWS_NN_WAVES - 1] if K >= 3 else [item_rows + 1]
        if B < sum(counts) + 1:
            return None
        m = np.full(B, POOL_NONE, np.uint32)
        at = np.random.default_rng(1000 + seed).permutation(B)
        pos = 0
        for k, c in enumerate(counts):
            m[at[pos:pos + c]] = k
            pos += c
        return m
    raise ValueError(kind)


def items_and_rows(member, K, item_rows):
    """csrc/kws_pool.cpp's kws_pool_items restated: ([(member, first position in the packed row list, count)], the packed row list) -- every
    named member's rows ascending, member after member, each list cut every item_rows rows; a member nobody names has no item"""
    items, rows = [], []
    for k in range(K):
        mine = [i for i, m in enumerate(member) if int(m) == k]
        for p in range(0, len(mine), item_rows):
            items.append((k, len(rows) + p, min(item_rows, len(mine) - p)))
        rows += mine
    return items, rows


def expected_bits(member, own, rows, stride):
    """the bits a pool call must leave in a [rows][stride] matrix prefilled with the sentinel: row i < len(member) holds, in its member's
    label columns, own[member][i] (the member's own entry point on every row of the call); every other word is the sentinel still"""
    want = np.full((rows, stride), SENTINEL_BITS, np.uint32)
    member = np.asarray(member, np.uint32)
    for k in np.unique(member[member != POOL_NONE]):
        at = np.nonzero(member == k)[0]
        labels = own[int(k)].shape[1]
        want[at, :labels] = bits(own[int(k)])[at]
        assert (want[at, :labels] != SENTINEL_BITS).all(), ("the member's own call left a row unwritten", int(k))
    return want


def check_scores(got, member, own, what):
    """got [rows][stride] (numpy float32) against expected_bits: named rows in bits against the member's own call, the rest the sentinel"""
    want = expected_bits(member, own, got.shape[0], got.shape[1])
    bad = np.argwhere(bits(got) != want)
    assert bad.size == 0, (what, "first differing (row, column):", bad[:4].tolist())
