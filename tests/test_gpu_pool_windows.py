"""Pools over windows on the GPU (kws_pool_scan_recordings_device, kws_pool_slide_recordings_device, kws_pool_slide_live_*,
kws_pool_cmvn_inference_device; the contract is in include/kws/kws.h) on the synthetic tenants of tests/pool_testlib.py.  Every output is
filled with the bit pattern 0x7fc0dead before each call, two rows past the call included.  A named window's row must hold, in its member's
label columns, the bits of that member's own entry point on that recording, stream or row alone and, on at most 64 windows per case, the
oracle's; every other word must still be the sentinel; `features` must be the first member's own call's bits for every window.  Bits only:
no tolerance anywhere."""
import sys

import numpy as np
import pytest

from kws_testlib import ROOT, OracleModel, bits, special_clips
from pool_testlib import KWS_NN_WAVES, PATTERNS, POOL_NONE, SENTINEL_BITS, check_scores, load_tenants, pattern, write_tenants
from scan_testlib import moving_average, oracle_scan, pack, speech
from slide_testlib import cut_windows

pytestmark = pytest.mark.gpu

CLIP = 16000
STRIDE = 320                   # the frame stride of the tenants' DSP blocks, in samples
TAPS = 2                       # EI_CLASSIFIER_SLICES_PER_MODEL_WINDOW >> 1
AUTO, DIRECT, SHARED = 0, 1, 2
K_MAX = 17                     # one above a bank's limit
ORACLE_ROWS = 64
PAD = 2                        # rows past the call in every output: they must stay the sentinel
NOBODY = 1                     # the member no recording of the mix names


@pytest.fixture(scope="module")
def pkg():
    sys.path.insert(0, ROOT)
    import torch  # noqa: F401
    from __graft_entry__ import load_package
    return load_package()


@pytest.fixture(scope="module")
def tenants(pkg, oracle, tmp_path_factory):
    """width -> ([loaded model], [oracle model]) of K_MAX tenants, and (width, K) -> the pool over the first K of them; made once"""
    directory = tmp_path_factory.mktemp("pool_windows_tenants")
    made, pools = {}, {}

    def models(width):
        if width not in made:
            paths = write_tenants(directory, width, K_MAX)
            made[width] = (load_tenants(pkg, paths), [OracleModel(oracle, p) for p in paths])
        return made[width]

    def pool(width, K):
        if (width, K) not in pools:
            pools[(width, K)] = pkg.Pool(models(width)[0][:K])
        return pools[(width, K)]

    yield models, pool
    for p in pools.values():
        p.close()
    for gms, _ in made.values():
        for gm in gms:
            gm.close()


def sentinel(rows, cols):
    import torch
    return torch.full((rows, cols), SENTINEL_BITS, dtype=torch.int32, device="cuda").view(torch.float32)


def host(t):
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy()


def same(a, b):
    return a.shape == b.shape and bool((bits(a) == bits(b)).all())


def untouched(a):
    return bool((bits(a) == SENTINEL_BITS).all())


def mix(K, item_rows):
    """(window counts, members) of the nine recordings of the scan and slide cases: 0 samples and too short for a window; one, two (= taps),
    taps + 1 and 23 windows; a KWS_POOL_NONE recording with windows and one without; member NOBODY unnamed; member 0 in three non-adjacent
    recordings with exactly item_rows windows in all; member 2 in two with item_rows + 1; member 3 with fewer than KWS_NN_WAVES; the last
    member of the pool (beyond a bank's sixteen at K = 17) with taps windows"""
    W = [0, 0, 1, 2, TAPS + 1, 23, item_rows - 2, item_rows, TAPS]
    member = np.array([POOL_NONE, 0, 2, 0, 3, POOL_NONE, 0, 2, K - 1], np.uint32)
    return W, member


def check_mix(W, member, K, item_rows):
    total = lambda k: sum(w for w, m in zip(W, member) if m == k)
    assert total(0) == item_rows and total(2) == item_rows + 1 and 0 < total(3) < KWS_NN_WAVES and total(K - 1) == TAPS
    assert not (member == NOBODY).any() and W[0] == W[1] == 0 and member[0] == POOL_NONE and member[5] == POOL_NONE and W[5] == 23
    at0 = np.nonzero(member == 0)[0]
    assert at0.size == 3 and (np.diff(at0) > 1).all() and {1, 2, TAPS, TAPS + 1} <= set(W)
    assert total(POOL_NONE) == 23


def test_the_recording_mix_is_what_it_says():
    """the inputs of the GPU cases, checked as arithmetic (no device work), for any item size"""
    for item_rows in (4, 16, 64):
        for K in (5, 17):
            W, member = mix(K, item_rows)
            check_mix(W, member, K, item_rows)
    assert sum(mix(17, 16)[0]) - 23 <= ORACLE_ROWS               # the named windows of a case, all checked against the oracle


def expected_rows(W, member, own, stride):
    """[sum W + PAD][stride] bits: recording r's rows hold own[r] (its member's own call on it alone) in that member's label columns"""
    want = np.full((sum(W) + PAD, stride), SENTINEL_BITS, np.uint32)
    cut = np.cumsum([0] + list(W))
    for r, o in own.items():
        assert o.shape[0] == W[r] and not (bits(o) == SENTINEL_BITS).any()
        want[cut[r]:cut[r + 1], :o.shape[1]] = bits(o)
    return want


def assert_bits(got, want, what):
    bad = np.argwhere(bits(got) != want)
    assert bad.size == 0, (what, "first differing (row, column):", bad[:4].tolist())


# ---- recording scans -----------------------------------------------------------------------------------------------------------------
def other_slicing(pkg, gm):
    """a slicing other than the quarter clip that the scan layout accepts"""
    for cand in (2000, 8000, 1000):
        try:
            gm.scan_window_count(CLIP, cand)
            return cand
        except pkg.KwsError:
            pass
    raise AssertionError("no second slicing")


@pytest.mark.parametrize("width,K", [("49x13", 5), ("49x13", 17), ("49x40", 5)])
def test_pool_scan_matches_each_member_and_the_oracle(width, K, pkg, oracle, tenants):
    import torch
    gms, oms = tenants[0](width)
    pool = tenants[1](width, K)
    item_rows, stride = pool.L.kws_pool_item_rows(), pool.score_stride
    W, member = mix(K, item_rows)
    check_mix(W, member, K, item_rows)
    R, n = len(W), sum(W)
    for sl in (CLIP // 4, other_slicing(pkg, gms[0])):
        k1 = next(k for k in range(1, 64) if gms[0].scan_window_count(k * sl, sl))          # slices up to the first window
        tails = [0, sl - 1, 1, 321, 0, sl - 1, 17, 0, 320]
        lens = [0, (k1 - 1) * sl + tails[1]] + [(w + k1 - 1) * sl + t for w, t in zip(W[2:], tails[2:])]
        recs = [speech(oracle, 1400 + i, x) for i, x in enumerate(lens)]
        pcm, offs, lens = pack(recs, seed=21, max_gap=9)
        assert [gms[0].scan_window_count(int(x), sl) for x in lens] == W
        # aligned and odd sample offsets: the buffer is shifted so that recording 5 starts on a 16-byte boundary
        shift = int(-int(offs[5]) % 8)
        pcm = np.concatenate([np.full(shift, 12345, np.int16), pcm])
        offs = offs + np.uint64(shift)
        assert int(offs[5]) % 8 == 0 and sum(int(o) % 8 != 0 for o in offs) >= 4
        d = torch.from_numpy(pcm).cuda()
        own_s, own_r = {}, {}
        for r in range(R):
            if member[r] == POOL_NONE or not W[r]:
                continue
            gm = gms[int(member[r])]
            so, ro = sentinel(W[r] + PAD, gm.n_labels), sentinel(W[r] + PAD, gm.n_labels)
            gm.scan_recordings_device(d.data_ptr(), offs[r:r + 1], lens[r:r + 1], so.data_ptr(), ro.data_ptr(), slice_samples=sl)
            so, ro = host(so), host(ro)
            assert untouched(so[W[r]:]) and same(moving_average(ro[:W[r]], TAPS), so[:W[r]])
            assert same(so[:W[r]], oracle_scan(oms[int(member[r])], recs[r], sl)), (width, K, sl, r, "the member's own scan is the oracle's")
            own_s[r], own_r[r] = so[:W[r]], ro[:W[r]]
        assert len(own_s) == 6
        want_s, want_r = expected_rows(W, member, own_s, stride), expected_rows(W, member, own_r, stride)
        for raw in (True, False):
            s, r = sentinel(n + PAD, stride), sentinel(n + PAD, stride)
            pool.scan_recordings_device(d.data_ptr(), offs, lens, member, s.data_ptr(), r.data_ptr() if raw else None, slice_samples=sl)
            s, r = host(s), host(r)
            assert_bits(s, want_s, (width, K, sl, raw, "scores"))
            if raw:
                assert_bits(r, want_r, (width, K, sl, "raw_scores"))
            else:
                assert untouched(r)
        # every recording names nobody: OK, nothing written
        s, r = sentinel(n + PAD, stride), sentinel(n + PAD, stride)
        pool.scan_recordings_device(d.data_ptr(), offs, lens, np.full(R, POOL_NONE, np.uint32), s.data_ptr(), r.data_ptr(), slice_samples=sl)
        assert untouched(host(s)) and untouched(host(r))
        # an index at or above K, on a recording without windows too: refused with the recording named, nothing written
        for at in (R - 1, 1):
            bad = member.copy()
            bad[at] = K
            with pytest.raises(pkg.KwsError) as e:
                pool.scan_recordings_device(d.data_ptr(), offs, lens, bad, s.data_ptr(), r.data_ptr(), slice_samples=sl)
            assert e.value.code == -20 and "recording %d:" % at in str(e.value) and untouched(host(s)) and untouched(host(r))


# ---- slides ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hop,flag", [(5 * STRIDE, SHARED), (1 + STRIDE, DIRECT)], ids=["hop_on_the_stride", "hop_off_the_stride"])
@pytest.mark.parametrize("width,K", [("49x13", 5), ("49x13", 17), ("49x40", 5)])
def test_pool_slide_matches_each_member_and_the_oracle(width, K, hop, flag, pkg, oracle, tenants):
    import torch
    gms, oms = tenants[0](width)
    pool = tenants[1](width, K)
    assert gms[0].frame_stride_samples == STRIDE
    item_rows, stride, F = pool.L.kws_pool_item_rows(), pool.score_stride, gms[0].n_features
    W, member = mix(K, item_rows)
    check_mix(W, member, K, item_rows)
    R, n = len(W), sum(W)
    tails = [0, 0, 0, hop - 1, 1, 5, 0, hop - 1, 3]
    lens = [0, CLIP - 1] + [CLIP + (w - 1) * hop + t for w, t in zip(W[2:], tails[2:])]
    recs = [speech(oracle, 1500 + i, x) for i, x in enumerate(lens)]
    pcm, offs, lens = pack(recs, seed=23, max_gap=9)
    shift = int(-int(offs[5]) % 8)
    pcm = np.concatenate([np.full(shift, 12345, np.int16), pcm])
    offs = offs + np.uint64(shift)
    assert int(offs[5]) % 8 == 0 and sum(int(o) % 8 != 0 for o in offs) >= 4
    assert [gms[0].slide_window_count(int(x), hop) for x in lens] == W
    assert (gms[0].slide_plan(lens, hop)["path"] == SHARED) == (hop % STRIDE == 0)
    d = torch.from_numpy(pcm).cuda()
    windows, Wc = cut_windows(recs, CLIP, hop)
    assert Wc == W
    cut = np.cumsum([0] + W)
    own = {}
    for r in range(R):
        if member[r] == POOL_NONE or not W[r]:
            continue
        k = int(member[r])
        so = sentinel(W[r] + PAD, gms[k].n_labels)
        gms[k].slide_recordings_device(d.data_ptr(), offs[r:r + 1], lens[r:r + 1], hop, so.data_ptr(), None)
        so = host(so)
        assert untouched(so[W[r]:])
        assert same(so[:W[r]], oms[k].run_batch(windows[cut[r]:cut[r + 1]])), (width, K, hop, r, "the member's own slide is the oracle's")
        own[r] = so[:W[r]]
    assert len(own) == 6
    want = expected_rows(W, member, own, stride)
    # the first member's own slide over every recording: the features of every window
    s0, f0 = sentinel(n + PAD, gms[0].n_labels), sentinel(n + PAD, F)
    gms[0].slide_recordings_device(d.data_ptr(), offs, lens, hop, s0.data_ptr(), f0.data_ptr())
    f0 = host(f0)
    assert untouched(f0[n:]) and not (bits(f0[:n]) == SENTINEL_BITS).all(axis=1).any()
    for flags in (AUTO, flag):
        for with_features in (True, False):
            s, f = sentinel(n + PAD, stride), sentinel(n + PAD, F)
            pool.slide_recordings_device(d.data_ptr(), offs, lens, member, hop, s.data_ptr(), f.data_ptr() if with_features else None, flags=flags)
            s, f = host(s), host(f)
            assert_bits(s, want, (width, K, hop, flags, with_features))
            assert same(f, f0) if with_features else untouched(f), (width, K, hop, flags)
    # features alone; every recording names nobody: nothing of scores is written
    s, f = sentinel(n + PAD, stride), sentinel(n + PAD, F)
    pool.slide_recordings_device(d.data_ptr(), offs, lens, member, hop, None, f.data_ptr())
    assert same(host(f), f0)
    pool.slide_recordings_device(d.data_ptr(), offs, lens, np.full(R, POOL_NONE, np.uint32), hop, s.data_ptr(), None)
    assert untouched(host(s))
    bad = member.copy()
    bad[1] = K                                                   # (a recording shorter than a clip: its member is still checked)
    with pytest.raises(pkg.KwsError) as e:
        pool.slide_recordings_device(d.data_ptr(), offs, lens, bad, hop, s.data_ptr(), None)
    assert e.value.code == -20 and "recording 1:" in str(e.value) and untouched(host(s))
    with pytest.raises(pkg.KwsError) as e:
        pool.slide_recordings_device(d.data_ptr(), offs, lens, member, hop, None, None)
    assert e.value.code == -20


# ---- live one-shot windows ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", [SHARED, DIRECT], ids=["shared", "direct"])
@pytest.mark.parametrize("width", ["49x13", "49x40"])
def test_pool_slide_streams_match_the_pool_slide_and_the_members_own_sessions(width, flags, pkg, oracle, tenants):
    """S = 12, K = 5: empty pushes, pushes shorter than a hop and long ones at unaligned offsets; stream 11 stays unassigned; stream 4 gets
    another member between two pushes; stream 3 is reset and keeps its member"""
    import torch
    gms, oms = tenants[0](width)
    K, S, hop = 5, 12, 5 * STRIDE
    pool = tenants[1](width, K)
    stride, F = pool.score_stride, gms[0].n_features
    sl = pool.slide_streams(S, hop, flags)
    own = [gm.slide_streams(S, hop, flags) for gm in gms[:K]]
    try:
        assert sl.path == flags and all(o.path == flags for o in own)
        assign = np.full(S, POOL_NONE, np.uint32)
        recs = [speech(oracle, 1600 + s, CLIP + 9 * hop + 11 + s) for s in range(S)]
        heard = [np.zeros(0, np.int16) for _ in range(S)]        # the audio of each stream since its start
        rows = [[] for _ in range(S)]                            # per stream: (score row bits, member at the time)
        pos = [0] * S
        oracle_left = [ORACLE_ROWS]

        def set_members(streams, member):
            sl.assign(streams, member)
            assign[list(streams)] = member

        def take(s, n):
            c = recs[s][pos[s]:pos[s] + n]
            pos[s] += c.size
            return c

        def push(entries, seed):
            streams = [e[0] for e in entries]
            chunks = [e[1] for e in entries]
            want = [sl.window_count(s, c.size) for s, c in zip(streams, chunks)]
            n = sum(want)
            pcm, offs, lens = pack(chunks, seed=seed, max_gap=9)
            assert any(int(o) % 8 for o in offs)
            d = torch.from_numpy(pcm).cuda()
            sc, ft = sentinel(n + PAD, stride), sentinel(n + PAD, F)
            nw = sl.push_device(d.data_ptr(), streams, offs, lens, sc.data_ptr(), ft.data_ptr())
            assert [int(x) for x in nw] == want                  # n_windows equals window_count
            sc, ft = host(sc), host(ft)
            member = np.repeat(assign[streams], want).astype(np.uint32)
            so_all, f_own = [], None
            for k, o in enumerate(own):
                so, fo = sentinel(max(n, 1), gms[k].n_labels), sentinel(n + PAD, F)
                nwo = o.push_device(d.data_ptr(), streams, offs, lens, so.data_ptr(), fo.data_ptr() if k == 0 else None)
                assert [int(x) for x in nwo] == want
                so_all.append(host(so)[:n])
                f_own = host(fo) if k == 0 else f_own
            check_scores(sc, member, so_all, ("scores", width, flags, streams))
            assert same(ft, f_own), ("features", width, flags, streams)
            at = 0
            for s, c, w in zip(streams, chunks, want):
                heard[s] = np.concatenate([heard[s], c])
                rows[s] += [(bits(sc[at + i]), int(assign[s])) for i in range(w)]
                at += w
            return want

        set_members(range(S - 1), [s % K for s in range(S - 1)])
        assert push([(s, take(s, CLIP - 1)) for s in range(S)], seed=1) == [0] * S                         # no window yet
        assert push([(s, take(s, 1 + hop)) for s in range(S)], seed=2) == [2] * S
        # a stream named twice: refused, nothing written, nothing advanced
        sc = sentinel(8, stride)
        d = torch.from_numpy(np.zeros(3 * hop + 8, np.int16)).cuda()
        with pytest.raises(pkg.KwsError) as e:
            sl.push_device(d.data_ptr(), [2, 5, 2], [1, 1, 1], [hop] * 3, sc.data_ptr(), None)
        assert e.value.code == -20 and "entry 2: stream 2 named twice" in str(e.value) and untouched(host(sc))
        set_members([4], [0])                                    # stream 4 was member 4's: from here on its rows are member 0's
        w = push([(11, take(11, 3 * hop)), (4, take(4, 2 * hop + 5)), (0, take(0, 100)), (7, take(7, 0)), (2, take(2, 4 * hop + 5))], seed=3)
        assert w == [3, 2, 0, 0, 4]
        sl.reset([3])                                            # stream 3 starts over with its member
        for o in own:
            o.reset([3])
        heard[3], rows[3], pos[3] = np.zeros(0, np.int16), [], 0
        w = push([(3, take(3, CLIP + 2 * hop)), (4, take(4, hop - 5)), (0, take(0, hop - 100)), (9, take(9, 0))], seed=4)
        assert w == [3, 1, 1, 0]
        push([(s, take(s, recs[s].size)) for s in (0, 1, 2, 4, 5, 11)], seed=5)
        assert assign[3] == 3 and assign[11] == POOL_NONE and {m for _, m in rows[4]} == {4, 0} and len(rows[3]) == 3
        # every stream's rows against the pool slide over its audio, window w under the member it had at the time; and the oracle
        n_checked = 0
        for s in range(S):
            n = len(rows[s])
            assert n == gms[0].slide_window_count(heard[s].size, hop) and n > 0
            pcm, offs, lens = pack([heard[s]], seed=40 + s, max_gap=9)
            d = torch.from_numpy(pcm).cuda()
            for m in sorted({m for _, m in rows[s]}):
                out = sentinel(n + PAD, stride)
                pool.slide_recordings_device(d.data_ptr(), offs, lens, np.array([m], np.uint32), hop, out.data_ptr(), None, flags=flags)
                out = bits(host(out))
                assert (out[n:] == SENTINEL_BITS).all()
                at = [i for i, (_, mm) in enumerate(rows[s]) if mm == m]
                assert all((rows[s][i][0] == out[i]).all() for i in at), (width, flags, s, m)
                if m != POOL_NONE and oracle_left[0] >= len(at):
                    oracle_left[0] -= len(at)
                    win, _ = cut_windows([heard[s]], CLIP, hop)
                    ref = bits(oms[m].run_batch(win[at]))
                    assert all((rows[s][i][0][:ref.shape[1]] == ref[j]).all() for j, i in enumerate(at)), (width, flags, s, m, "oracle")
                    n_checked += len(at)
        assert n_checked >= 32
    finally:
        sl.close()
        for o in own:
            o.close()


# ---- cepstra in ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cepstra_case(tenants, oracle):
    """width -> 203 cepstral matrices (the first member's mfcc_batch_device) on the device, each tenant's own cmvn_inference_batch_device
    rows, the first tenant's features and the clips; computed once"""
    made = {}

    def get(width):
        import torch
        if width not in made:
            gms, _ = tenants[0](width)
            B, F = 203, gms[0].n_features
            sp = np.stack(list(special_clips().values()))
            clips = np.concatenate([sp, oracle.synth(43, 0, B - sp.shape[0])])
            mfcc = torch.empty((B, F), dtype=torch.float32, device="cuda")
            gms[0].mfcc_batch_device(torch.from_numpy(clips).cuda().data_ptr(), B, mfcc.data_ptr())
            own, f0 = [], sentinel(B, F)
            for k, gm in enumerate(gms):
                so = sentinel(B, gm.n_labels)
                gm.cmvn_inference_batch_device(mfcc.data_ptr(), B, so.data_ptr(), f0.data_ptr() if k == 0 else None)
                own.append(host(so))
            f0 = host(f0)
            for a in own + [f0, clips]:
                a.setflags(write=False)
            made[width] = (mfcc, own, f0, clips)
        return made[width]

    return get


@pytest.mark.parametrize("B", [1, 9, 203])
@pytest.mark.parametrize("width,K", [("49x13", 17), ("49x40", 5)])
def test_pool_cepstra_in_matches_each_member_and_the_oracle(width, K, B, pkg, tenants, cepstra_case):
    gms, oms = tenants[0](width)
    pool = tenants[1](width, K)
    mfcc, own, f0, clips = cepstra_case(width)
    stride, F = pool.score_stride, gms[0].n_features
    item_rows = pool.L.kws_pool_item_rows()
    ran = []
    for kind in PATTERNS:
        member = pattern(kind, B, K, item_rows, seed=B + K)
        if member is None:
            continue
        ran.append(kind)
        for with_features in (True, False):
            s, f = sentinel(B + PAD, stride), sentinel(B + PAD, F)
            pool.cmvn_inference_device(mfcc.data_ptr(), B, member, s.data_ptr(), f.data_ptr() if with_features else None)
            s, f = host(s), host(f)
            check_scores(s, member, own, (width, K, B, kind))
            assert (same(f[:B], f0[:B]) and untouched(f[B:])) if with_features else untouched(f), (width, K, B, kind)
        if kind == "robin":
            m = min(B, ORACLE_ROWS)
            for k in sorted(set(int(x) for x in member[:m])):
                at = [i for i in range(m) if member[i] == k]
                assert same(s[at, :gms[k].n_labels], oms[k].run_batch(clips[at])), (width, K, B, "oracle", k)
    assert {"one", "robin", "none", "never"} <= set(ran) and (B < 203 or set(ran) == set(PATTERNS))
    bad = pattern("robin", B, K, item_rows)
    bad[B - 1] = K
    t = sentinel(B, stride)
    with pytest.raises(pkg.KwsError) as e:
        pool.cmvn_inference_device(mfcc.data_ptr(), B, bad, t.data_ptr(), None)
    assert e.value.code == -20 and "row %d:" % (B - 1) in str(e.value) and untouched(host(t))


# ---- more windows than one chunk of the finishing step --------------------------------------------------------------------------------
def test_pool_window_calls_over_two_chunks_of_the_finishing_step(pkg, tenants):
    """The finishing step takes at most 64 MiB of gathered windows at a time: 8 559 windows of 49 x 40 features.  Twelve recordings of 714
    windows (8 568) span two chunks -- the second chunk's member table, row offset and upload, a wbase that spans chunks -- in one scan, one
    slide and one live one-shot push, each compared with the same audio in two calls of six recordings that fit one chunk each."""
    import torch
    pool = tenants[1]("49x40", 5)
    gm = pool.members[0]
    F, stride = gm.n_features, pool.score_stride
    chunk = (64 << 20) // (4 * F)
    R, sl, per = 12, 4000, 714
    assert 11 * per <= chunk < R * per and 6 * per <= chunk
    n1 = (per + 3) * sl
    assert gm.scan_window_count(n1, sl) == per and gm.slide_window_count(n1, sl) == per
    d = torch.empty((R, n1), dtype=torch.int16, device="cuda")
    pkg.synth_clips_device(94, 0, R, n1, d.data_ptr())
    member = np.array([r % 5 for r in range(R)], np.uint32)
    member[7] = POOL_NONE
    offs, lens = np.array([r * n1 for r in range(R)], np.uint64), np.full(R, n1, np.uint64)
    n, h = R * per, 6 * per
    labels = [0 if m == POOL_NONE else pool.members[int(m)].n_labels for m in member]

    def check(whole, halves, what):
        torch.cuda.synchronize()
        got = whole.view(torch.int32)
        want = torch.cat([halves[0].view(torch.int32)[:h], halves[1].view(torch.int32)[:h]])
        assert bool((got[:n] == want).all()) and bool((got[n:] == SENTINEL_BITS).all()), what
        for r in range(R):
            rows = got[r * per:(r + 1) * per]
            assert bool((rows[:, labels[r]:] == SENTINEL_BITS).all()) and (not labels[r] or bool((rows[:, :labels[r]] != SENTINEL_BITS).all())), (what, r)

    # the scan, with raw scores
    a, ra = sentinel(n + PAD, stride), sentinel(n + PAD, stride)
    pool.scan_recordings_device(d.data_ptr(), offs, lens, member, a.data_ptr(), ra.data_ptr(), slice_samples=sl)
    b, rb = [sentinel(h + PAD, stride) for _ in range(2)], [sentinel(h + PAD, stride) for _ in range(2)]
    for i in range(2):
        pool.scan_recordings_device(d.data_ptr(), offs[6 * i:6 * i + 6], lens[6 * i:6 * i + 6], member[6 * i:6 * i + 6], b[i].data_ptr(), rb[i].data_ptr(), slice_samples=sl)
    check(a, b, "scan")
    check(ra, rb, "scan raw")
    # the slide at a hop of one slice
    a = sentinel(n + PAD, stride)
    pool.slide_recordings_device(d.data_ptr(), offs, lens, member, sl, a.data_ptr(), None)
    b = [sentinel(h + PAD, stride) for _ in range(2)]
    for i in range(2):
        pool.slide_recordings_device(d.data_ptr(), offs[6 * i:6 * i + 6], lens[6 * i:6 * i + 6], member[6 * i:6 * i + 6], sl, b[i].data_ptr(), None)
    check(a, b, "slide")
    slide_rows = a
    # one live one-shot push of twelve streams, against two pushes of six
    one, two = pool.slide_streams(R, sl), pool.slide_streams(R, sl)
    try:
        streams = list(range(R))
        one.assign(streams, member)
        two.assign(streams, member)
        a = sentinel(n + PAD, stride)
        nw = one.push_device(d.data_ptr(), streams, offs, lens, a.data_ptr(), None)
        assert [int(x) for x in nw] == [per] * R
        b = [sentinel(h + PAD, stride) for _ in range(2)]
        for i in range(2):
            nw = two.push_device(d.data_ptr(), streams[6 * i:6 * i + 6], offs[6 * i:6 * i + 6], lens[6 * i:6 * i + 6], b[i].data_ptr(), None)
            assert [int(x) for x in nw] == [per] * 6
        check(a, b, "live one-shot")
        assert bool((a.view(torch.int32) == slide_rows.view(torch.int32)).all())
    finally:
        one.close()
        two.close()
