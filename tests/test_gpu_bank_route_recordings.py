"""Routed recording scans, slides and cepstra-in bank calls on the GPU (kws_bank_scan_recordings_routed_device,
kws_bank_slide_recordings_routed_device, kws_bank_cmvn_inference_routed_device; the contract is in include/kws/kws.h) on two banks: the
four 49x40 models, whose network kernels differ (matrix-core int8 at 64-byte rows, a class-2 int8 DS-CNN, two float graphs), and the 49x13
bank of tests/test_gpu_bank_windows.py, whose label counts differ (2, 2, 3 and 5).  The sentinel discipline is tests/test_gpu_bank_route.py's:
every score buffer is filled with the bit pattern 0x7fc0dead before each call; a routed (window, member) pair's row must be the bits of the
member's own entry point in KWS_MODE_EXACT and, on up to 64 rows, match the oracle (int8 bit-exact, float32 scores within 1e-6); every
other row must still hold the sentinel bits; `features` must be the unrouted call's bits.

No case is vacuous, as a condition on the inputs asserted before each call: outside the route kinds that rule it out by their definition
(all members; one member never named; only the last recording routed), every member has at least one routed and one unrouted recording
THAT HAS WINDOWS (a row, for the cepstra-in call)."""
import os
import sys

import numpy as np
import pytest

from kws_testlib import MODELS, ROOT, OracleModel, bits, special_clips, synth_model_blob
from scan_testlib import moving_average, oracle_scan, pack, speech
from slide_testlib import cut_windows
from test_gpu_bank import _blob
from test_gpu_bank_route import KINDS, MFCC40, SENTINEL_BITS, assert_not_vacuous, make_routes, routed
from test_gpu_bank_windows import BANKS as WINDOW_BANKS, SYNTH13_L5

pytestmark = pytest.mark.gpu

F32_SCORE_TOL = 1e-6           # the project's bar for exact-mode float32 scores
CLIP = 16000
STRIDE = 320                   # the frame stride of both banks' DSP blocks, in samples
AUTO, DIRECT, SHARED = 0, 1, 2
BANKS = {"49x40": MFCC40, "49x13": WINDOW_BANKS["49x13"]}
ORACLE_ROWS = 64
CHUNK_49x40 = 8559             # kws_window_chunk(1960, .): the windows of one gather chunk at F = 1960 (csrc/kws_windows.h)
SCAN_SLICES = [4, 7, 12, 5, 9, 3, 6, 1, 10]           # slices per recording at k_full = 3: recordings 5 and 7 have no window
SCAN_TAILS = [1, 3999, 321, 0, 1777, 3999, 17, 0, 320]  # trailing partial slices, in samples


@pytest.fixture(scope="module")
def pkg():
    sys.path.insert(0, ROOT)
    import torch  # noqa: F401
    from __graft_entry__ import load_package
    return load_package()


@pytest.fixture(scope="module")
def banks(pkg, oracle, tmp_path_factory):
    """bank name -> (Bank, [(product model, oracle model)]), created once per module"""
    models, made = {}, {}
    tmp = tmp_path_factory.mktemp("bank_route_recordings")

    def model(name):
        if name not in models:
            path = os.path.join(MODELS, name)
            if not name.endswith(".kwsm"):
                path = str(tmp / (name + ".kwsm"))
                open(path, "wb").write(synth_model_blob(**SYNTH13_L5) if name == "synth13_l5" else _blob(name))
            models[name] = (pkg.Model(path), OracleModel(oracle, path))
        return models[name]

    def get(name):
        if name not in made:
            members = [model(n) for n in BANKS[name]]
            made[name] = (pkg.Bank([gm for gm, _ in members]), members)
        return made[name]

    yield get
    for bank, _ in made.values():
        bank.close()
    for gm, _ in models.values():
        gm.close()


def sentinel(rows, cols):
    import torch
    return torch.full((rows, cols), SENTINEL_BITS, dtype=torch.int32, device="cuda").view(torch.float32)


def outputs(gms, rows):
    return [sentinel(rows, gm.n_labels) for gm in gms]


def ptrs(tensors, skip=()):
    return [None if k in skip else t.data_ptr() for k, t in enumerate(tensors)]


def host(tensors):
    import torch
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in tensors]


def same(a, b):
    return a.shape == b.shape and bool((bits(a) == bits(b)).all())


def untouched(a):
    return bool((bits(a) == SENTINEL_BITS).all())


def check_member(got, want, mask, what):
    """rows of `mask`: the bits of `want`; every other row (the margin behind the call's rows included): the sentinel bits"""
    n = mask.size
    assert same(got[:n][mask], want[:n][mask]), what
    assert untouched(got[:n][~mask]) and untouched(got[n:]), what


def check_oracle(got, want, is_float, what):
    if not got.size:
        return
    if is_float:
        err = float(np.abs(got - want).max())
        print("%s: max |score - oracle| %.3g" % (what, err))
        assert err <= F32_SCORE_TOL, (what, err)
    else:
        assert same(got, want), what


def window_mask(routes, W, k):
    """the rows of member k: a window's route is its recording's"""
    return np.repeat(routed(routes, k), W)


def check_routes(kind, routes, W, K, what):
    """the no-vacuity rule over the recordings that have windows (rows: W all ones); the degenerate kinds: what defines them"""
    act = np.asarray(routes)[np.asarray(W) > 0]
    if kind == "all":
        assert all(routed(act, k).all() for k in range(K)), what
    elif kind == "never":
        assert not routed(routes, 1).any() and (act != 0).all(), what
    elif kind == "last":
        assert int(np.count_nonzero(routes)) == 1 and routes[-1] == 1 << (K - 1) and W[-1] > 0, what
    else:
        assert_not_vacuous(act, K, what)
        assert kind != "random" or (act == 0).any(), what


def test_routes_of_every_case_meet_their_conditions():
    """the inputs of the GPU cases, checked as arithmetic (no device work)"""
    W_scan = [max(k - 3, 0) for k in SCAN_SLICES]
    assert W_scan.count(0) == 2 and W_scan[5] == 0 and W_scan[4] > 0 and W_scan[6] > 0 and W_scan[-1] > 0
    assert min(k for k in SCAN_SLICES if k > 3) == 4 and max(SCAN_SLICES) == 12 and sum(W_scan) <= ORACLE_ROWS
    W_slide = [1, 1, 2, 3, 1, 0, 2]
    for K in (4,):
        for kind in KINDS:
            check_routes(kind, make_routes(kind, len(W_scan), K, seed=9), W_scan, K, ("scan", kind))
            check_routes(kind, make_routes(kind, len(W_slide), K, seed=7), W_slide, K, ("slide", kind))
            for B in (9, 203):
                check_routes(kind, make_routes(kind, B, K, seed=B), [1] * B, K, ("cepstra", kind, B))


# ---- recording scans -----------------------------------------------------------------------------------------------------------------
def own_scan(gm, d, offs, lens, n, sl):
    s, r = sentinel(n + 2, gm.n_labels), sentinel(n + 2, gm.n_labels)
    gm.scan_recordings_device(d.data_ptr(), offs, lens, s.data_ptr(), r.data_ptr(), slice_samples=sl)
    return host([s, r])


def routed_scan(bank, d, offs, lens, routes, n, sl, raw=True, skip=()):
    gms = bank.members
    s, r = outputs(gms, n + 2), outputs(gms, n + 2)
    bank.scan_recordings_device(d.data_ptr(), offs, lens, ptrs(s, skip), ptrs(r, skip) if raw else None, slice_samples=sl, routes=routes)
    return host(s), host(r)


@pytest.fixture(scope="module")
def scan_case(banks, oracle):
    """bank name -> the scan's recordings on the device, their window counts, each member's own scan (scores, raw) and the oracle's scores of
    every window (32 of them), computed once and left unchanged"""
    made = {}

    def get(name):
        import torch
        if name not in made:
            bank, members = banks(name)
            gms = bank.members
            sl = 4000
            recs = [speech(oracle, 1200 + i, k * sl + t) for i, (k, t) in enumerate(zip(SCAN_SLICES, SCAN_TAILS))]
            pcm, offs, lens = pack(recs, seed=12, max_gap=9)
            assert sum(int(o) % 8 != 0 for o in offs) >= 6                      # unaligned sample offsets
            W = [gms[0].scan_window_count(int(x), sl) for x in lens]
            assert W == [max(k - 3, 0) for k in SCAN_SLICES] and all([gm.scan_window_count(int(x), sl) for x in lens] == W for gm in gms)
            d = torch.from_numpy(pcm).cuda()
            n = sum(W)
            own = [own_scan(gm, d, offs, lens, n, sl) for gm in gms]
            assert all(not untouched(o[0][:n]) and untouched(o[0][n:]) for o in own)
            ref = [np.concatenate([oracle_scan(om, rec, sl) for rec in recs]) for _, om in members]
            assert all(x.shape[0] == n for x in ref)
            for (gm, _), o, x in zip(members, own, ref):                        # the members' own scans are the reference's
                check_oracle(o[0][:n], x, gm.is_float, "%s own scan" % name)
                for a in (o[0], o[1], x):
                    a.setflags(write=False)
            made[name] = (d, offs, lens, W, own, ref, sl)
        return made[name]

    return get


@pytest.mark.parametrize("raw", [True, False], ids=["raw_scores", "in_place"])
@pytest.mark.parametrize("name", list(BANKS))
def test_routed_scan_matches_each_member_and_the_oracle(name, raw, pkg, banks, scan_case):
    """nine recordings of 1 to 12 slices with trailing partial slices at unaligned offsets, two of them too short for a window (one of
    those between two routed recordings), under every route kind; without raw_scores the filter works in place"""
    bank, members = banks(name)
    gms, K = bank.members, len(members)
    d, offs, lens, W, own, ref, sl = scan_case(name)
    n, R = sum(W), len(W)
    for kind in KINDS:
        routes = make_routes(kind, R, K, seed=9)
        check_routes(kind, routes, W, K, (name, kind))
        s, r = routed_scan(bank, d, offs, lens, routes, n, sl, raw=raw)
        for k, (gm, om) in enumerate(members):
            what = "%s / %s scan %s" % (name, BANKS[name][k], kind)
            mask = window_mask(routes, W, k)
            check_member(s[k], own[k][0], mask, what)
            if raw:
                check_member(r[k], own[k][1], mask, what + " raw")
            else:
                assert untouched(r[k]), what
            check_oracle(s[k][:n][mask], ref[k][mask], gm.is_float, what)
    if not raw:
        return
    # the moving average of a routed recording is the fresh filter over ITS raw rows, although unrouted recordings lie between them
    routes = make_routes("onehot", R, K)
    s, r = routed_scan(bank, d, offs, lens, routes, n, sl)
    cut = np.cumsum([0] + W)
    for k in range(K):
        for i in range(R):
            if W[i] and (routes[i] >> k) & 1:
                assert same(moving_average(r[k][cut[i]:cut[i + 1]]), s[k][cut[i]:cut[i + 1]]), (name, k, i)
    # a routed member without a score buffer is skipped: nothing is written for it, the other members' rows are what they were
    s3, r3 = routed_scan(bank, d, offs, lens, routes, n, sl, skip={0})
    assert untouched(s3[0]) and untouched(r3[0]) and window_mask(routes, W, 0).any()
    assert all(same(s3[k], s[k]) and same(r3[k], r[k]) for k in range(1, K))
    # routes == None is the unrouted call: every member's own rows
    s0, r0 = routed_scan(bank, d, offs, lens, None, n, sl)
    assert all(same(s0[k], own[k][0]) and same(r0[k], own[k][1]) for k in range(K))
    # one recording, routed to the last member alone
    i = 2
    one = np.array([1 << (K - 1)], np.uint32)
    s1, r1 = routed_scan(bank, d, offs[i:i + 1], lens[i:i + 1], one, W[i], sl)
    assert all(untouched(s1[k]) and untouched(r1[k]) for k in range(K - 1))
    check_member(s1[K - 1], own[K - 1][0][cut[i]:cut[i + 1]], np.ones(W[i], bool), (name, "R = 1"))
    check_member(r1[K - 1], own[K - 1][1][cut[i]:cut[i + 1]], np.ones(W[i], bool), (name, "R = 1 raw"))
    # a route bit at or above K: refused with the recording named, nothing written -- also where that recording has no window
    for at in (R - 1, 5):
        bad = make_routes("onehot", R, K)
        bad[at] |= 1 << K
        t = outputs(gms, n)
        with pytest.raises(pkg.KwsError) as e:
            bank.scan_recordings_device(d.data_ptr(), offs, lens, ptrs(t), None, slice_samples=sl, routes=bad)
        assert e.value.code == -20 and "recording %d:" % at in str(e.value) and "0x%x" % bad[at] in str(e.value) and all(untouched(x) for x in host(t))


def test_routed_scan_across_a_gather_chunk(pkg, banks):
    """three recordings of the 49x40 bank routed to members 0, 1 and 0, the boundary between two chunks of gathered windows strictly inside
    the second: the second chunk begins with rows of a member that has none at the end of the first and ends with a recording of another
    member; rows at row0 > 0 of the lists.  Against the members' own scans (the oracle is too slow for these counts)."""
    import torch
    bank, members = banks("49x40")
    gms, K = bank.members, len(members)
    # the shortest slicing the stream API accepts for these models keeps the audio small
    sl = None
    for cand in (2000, 4000):
        try:
            gms[0].scan_window_count(CLIP, cand)
            sl = cand
            break
        except pkg.KwsError:
            pass
    assert sl is not None
    k1 = next(k for k in range(1, 64) if gms[0].scan_window_count(k * sl, sl))          # slices up to the first window
    want_W = [CHUNK_49x40 - 300, 700, 50]
    lens = np.array([(w + k1 - 1) * sl + 7 * i for i, w in enumerate(want_W)], np.uint64)
    W = [gms[0].scan_window_count(int(x), sl) for x in lens]
    assert W == want_W and W[0] < CHUNK_49x40 < W[0] + W[1] and sum(W) > CHUNK_49x40
    offs = np.array([1, 1 + int(lens[0]) + 3, 1 + int(lens[0]) + 3 + int(lens[1]) + 5], np.uint64)
    total = int(offs[2] + lens[2])
    n_clips = (total + CLIP - 1) // CLIP
    big = torch.empty(n_clips * CLIP + 16, dtype=torch.int16, device="cuda")
    pkg.synth_clips_device(92, 0, n_clips, CLIP, big.data_ptr())
    torch.cuda.synchronize()
    routes = np.array([1, 2, 1], np.uint32)
    n = sum(W)
    s, r = outputs(gms, n + 1), outputs(gms, n + 1)
    bank.scan_recordings_device(big.data_ptr(), offs, lens, ptrs(s), ptrs(r), slice_samples=sl, routes=routes)
    torch.cuda.synchronize()
    for k, gm in enumerate(gms):
        mask = torch.from_numpy(np.concatenate([window_mask(routes, W, k), [False]])).cuda()
        if k > 1:
            assert not bool(mask.any())
        else:
            so, ro = sentinel(n + 1, gm.n_labels), sentinel(n + 1, gm.n_labels)
            gm.scan_recordings_device(big.data_ptr(), offs, lens, so.data_ptr(), ro.data_ptr(), slice_samples=sl)
            torch.cuda.synchronize()
            assert bool((so[:n].view(torch.int32) != SENTINEL_BITS).all())
            assert bool((s[k].view(torch.int32)[mask] == so.view(torch.int32)[mask]).all()), k
            assert bool((r[k].view(torch.int32)[mask] == ro.view(torch.int32)[mask]).all()), k
        assert bool((s[k].view(torch.int32)[~mask] == SENTINEL_BITS).all()) and bool((r[k].view(torch.int32)[~mask] == SENTINEL_BITS).all()), k


# ---- slides ------------------------------------------------------------------------------------------------------------------------
def slide_lengths(hop):
    """seven recordings around the window count's edges: exactly one clip, clip + hop - 1, clip + hop, shorter than a clip, ..."""
    return [CLIP, CLIP + hop - 1, CLIP + hop, CLIP + 2 * hop + 5, CLIP + 1, CLIP - 1, CLIP + 2 * hop - 1]


def routed_slide(bank, d, offs, lens, hop, flags, routes, n, want_features=True):
    gms = bank.members
    s, f = outputs(gms, n + 2), sentinel(n + 2, gms[0].n_features)
    bank.slide_recordings_device(d.data_ptr(), offs, lens, hop, ptrs(s), f.data_ptr() if want_features else None, flags=flags, routes=routes)
    return host(s), host([f])[0]


@pytest.mark.parametrize("hop", [5 * STRIDE, 1 + STRIDE], ids=["hop_on_the_stride", "hop_off_the_stride"])
@pytest.mark.parametrize("name", list(BANKS))
def test_routed_slide_matches_each_member_on_every_path(name, hop, pkg, oracle, banks):
    """a hop that is a multiple of the frame stride (AUTO picks SHARED) and one off it, flags AUTO, DIRECT and SHARED, every route kind,
    features requested: the paths stay bit-identical to each other under any routes"""
    import torch
    bank, members = banks(name)
    gms, K = bank.members, len(members)
    recs = [speech(oracle, 1300 + i, x) for i, x in enumerate(slide_lengths(hop))]
    pcm, offs, lens = pack(recs, seed=14, max_gap=9)
    d = torch.from_numpy(pcm).cuda()
    W = [gms[0].slide_window_count(int(x), hop) for x in lens]
    assert W == [1, 1, 2, 3, 1, 0, 2]
    n, R, F = sum(W), len(W), gms[0].n_features
    plan = gms[0].slide_plan(lens, hop)
    assert (plan["path"] == SHARED) == (hop % STRIDE == 0)
    # each member's own slide, and the unrouted bank call's features
    own = []
    for gm in gms:
        so = sentinel(n + 2, gm.n_labels)
        gm.slide_recordings_device(d.data_ptr(), offs, lens, hop, so.data_ptr(), None)
        own.append(host([so])[0])
    s0, f0 = routed_slide(bank, d, offs, lens, hop, AUTO, None, n)
    assert all(same(s0[k], own[k]) for k in range(K)) and untouched(f0[n:]) and not untouched(f0[:n])
    windows, Wc = cut_windows(recs, CLIP, hop)
    assert Wc == W
    ref = [om.run_batch(windows) for _, om in members]
    for kind in KINDS:
        routes = make_routes(kind, R, K, seed=7)
        check_routes(kind, routes, W, K, (name, hop, kind))
        for flags in (AUTO, DIRECT, SHARED):
            s, f = routed_slide(bank, d, offs, lens, hop, flags, routes, n)
            assert same(f, f0), (name, hop, kind, flags)
            for k, (gm, om) in enumerate(members):
                what = "%s / %s slide hop %d %s flags %d" % (name, BANKS[name][k], hop, kind, flags)
                mask = window_mask(routes, W, k)
                check_member(s[k], own[k], mask, what)
                if flags == AUTO:
                    check_oracle(s[k][:n][mask], ref[k][mask], gm.is_float, what)
    # without features: the same rows, nothing else written
    routes = make_routes("random", R, K, seed=7)
    s, f = routed_slide(bank, d, offs, lens, hop, AUTO, routes, n, want_features=False)
    assert untouched(f) and all(untouched(s[k][:n][~window_mask(routes, W, k)]) and same(s[k][:n][window_mask(routes, W, k)], own[k][:n][window_mask(routes, W, k)]) for k in range(K))
    bad = make_routes("onehot", R, K)
    bad[5] = 1 << K                                              # (a recording shorter than a clip: its route is still checked)
    t = outputs(gms, n)
    with pytest.raises(pkg.KwsError) as e:
        bank.slide_recordings_device(d.data_ptr(), offs, lens, hop, ptrs(t), None, routes=bad)
    assert e.value.code == -20 and "recording 5:" in str(e.value) and all(untouched(x) for x in host(t))


def test_routed_slide_across_a_gather_chunk(pkg, banks):
    """8 559 + 50 windows of the 49x40 bank at hop 160 over two recordings with different one-hot routes, the chunk boundary inside the
    first; against the members' own slides, features against the unrouted call's"""
    import torch
    bank, members = banks("49x40")
    gms, K = bank.members, len(members)
    hop = 160
    want_W = [CHUNK_49x40 + 20, 30]
    lens = np.array([CLIP + (w - 1) * hop + 3 for w in want_W], np.uint64)
    W = [gms[0].slide_window_count(int(x), hop) for x in lens]
    assert W == want_W and sum(W) == CHUNK_49x40 + 50
    offs = np.array([1, 1 + int(lens[0]) + 5], np.uint64)
    total = int(offs[1] + lens[1])
    n_clips = (total + CLIP - 1) // CLIP
    big = torch.empty(n_clips * CLIP + 16, dtype=torch.int16, device="cuda")
    pkg.synth_clips_device(93, 0, n_clips, CLIP, big.data_ptr())
    torch.cuda.synchronize()
    routes = np.array([1 << 2, 1 << 0], np.uint32)
    n, F = sum(W), gms[0].n_features
    s, f = outputs(gms, n + 1), sentinel(n + 1, F)
    bank.slide_recordings_device(big.data_ptr(), offs, lens, hop, ptrs(s), f.data_ptr(), routes=routes)
    s0, f0 = outputs(gms, n + 1), sentinel(n + 1, F)
    bank.slide_recordings_device(big.data_ptr(), offs, lens, hop, ptrs(s0), f0.data_ptr())
    torch.cuda.synchronize()
    assert bool((f.view(torch.int32) == f0.view(torch.int32)).all()) and bool((f0[:n].view(torch.int32) != SENTINEL_BITS).any())
    for k, gm in enumerate(gms):
        mask = torch.from_numpy(np.concatenate([window_mask(routes, W, k), [False]])).cuda()
        assert bool(mask.any()) == (k in (0, 2))
        if k in (0, 2):
            so = sentinel(n + 1, gm.n_labels)
            gm.slide_recordings_device(big.data_ptr(), offs, lens, hop, so.data_ptr(), None)
            torch.cuda.synchronize()
            assert bool((so[:n].view(torch.int32) != SENTINEL_BITS).all())
            assert bool((s[k].view(torch.int32)[mask] == so.view(torch.int32)[mask]).all()), k
        assert bool((s[k].view(torch.int32)[~mask] == SENTINEL_BITS).all()), k


# ---- cepstra in ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cepstra_case(banks, oracle):
    """bank name -> 203 cepstral matrices (kws_mfcc_batch_device of the first member) on the device, each member's own
    kws_cmvn_inference_batch_device rows, the unrouted bank call's features and the oracle's scores of the first 64 rows, computed once"""
    made = {}

    def get(name):
        import torch
        if name not in made:
            bank, members = banks(name)
            gms = bank.members
            B, F = 203, gms[0].n_features
            sp = np.stack(list(special_clips().values()))
            clips = np.concatenate([sp, oracle.synth(41, 0, B - sp.shape[0])])
            dc = torch.from_numpy(clips).cuda()
            mfcc = torch.empty((B, F), dtype=torch.float32, device="cuda")
            gms[0].mfcc_batch_device(dc.data_ptr(), B, mfcc.data_ptr())
            own = []
            for gm in gms:
                so = sentinel(B, gm.n_labels)
                gm.cmvn_inference_batch_device(mfcc.data_ptr(), B, so.data_ptr())
                own.append(so)
            s0, f0 = outputs(gms, B), sentinel(B, F)
            bank.cmvn_inference_batch_device(mfcc.data_ptr(), B, ptrs(s0), f0.data_ptr())
            own, s0, f0 = host(own), host(s0), host([f0])[0]
            assert all(same(a, b) and not untouched(a) for a, b in zip(s0, own))
            ref = [om.run_batch(clips[:ORACLE_ROWS]) for _, om in members]
            for (gm, _), o, x in zip(members, own, ref):
                check_oracle(o[:ORACLE_ROWS], x, gm.is_float, "%s own cepstra-in call" % name)
            made[name] = (mfcc, own, f0, ref)
        return made[name]

    return get


@pytest.mark.parametrize("B", [1, 9, 203])
@pytest.mark.parametrize("name", list(BANKS))
def test_routed_cepstra_in_matches_each_member_and_the_oracle(name, B, pkg, banks, cepstra_case):
    bank, members = banks(name)
    gms, K = bank.members, len(members)
    mfcc, own, f0, ref = cepstra_case(name)
    F = gms[0].n_features
    for kind in KINDS:
        routes = make_routes(kind, B, K, seed=B)
        if B > K:
            check_routes(kind, routes, [1] * B, K, (name, B, kind))
        for with_features in (True, False):
            s, f = outputs(gms, B + 2), sentinel(B + 2, F)
            bank.cmvn_inference_batch_device(mfcc.data_ptr(), B, ptrs(s), f.data_ptr() if with_features else None, routes=routes)
            s, f = host(s), host([f])[0]
            assert (same(f[:B], f0[:B]) and untouched(f[B:])) if with_features else untouched(f), (name, B, kind)
            for k, (gm, om) in enumerate(members):
                what = "%s / %s cepstra B %d %s" % (name, BANKS[name][k], B, kind)
                mask = routed(routes, k)
                check_member(s[k], own[k], mask, what)
                m = min(B, ORACLE_ROWS)
                check_oracle(s[k][:m][mask[:m]], ref[k][:m][mask[:m]], gm.is_float, what)
    # routes == None is the unrouted call
    s = outputs(gms, B + 2)
    bank.cmvn_inference_batch_device(mfcc.data_ptr(), B, ptrs(s), None, routes=None)
    assert all(same(a[:B], o[:B]) and untouched(a[B:]) for a, o in zip(host(s), own))
    bad = make_routes("onehot", B, K)
    bad[B - 1] |= 1 << K
    t = outputs(gms, B)
    with pytest.raises(pkg.KwsError) as e:
        bank.cmvn_inference_batch_device(mfcc.data_ptr(), B, ptrs(t), None, routes=bad)
    assert e.value.code == -20 and "row %d:" % (B - 1) in str(e.value) and all(untouched(x) for x in host(t))


# ---- the members stay as they were ------------------------------------------------------------------------------------------------
def test_routed_recording_calls_leave_the_members_untouched(pkg, oracle, banks, scan_case, cepstra_case):
    """the float32 member in KWS_MODE_FAST with a logits tap and counts from a fast call of its own: after routed calls in all three forms
    its mode, kws_fast_fallback_count, kws_fast_exact_count and tap are what they were, and the calls wrote the exact bits"""
    import torch
    bank, members = banks("49x13")
    gms, K = bank.members, len(members)
    gm = gms[1]
    assert gm.is_float
    d, offs, lens, W, own, ref, sl = scan_case("49x13")
    mfcc, own_c, f0, _ = cepstra_case("49x13")
    n, R, hop = sum(W), len(W), 5 * STRIDE
    n_slide = sum(gm.slide_window_count(int(x), hop) for x in lens)
    routes = np.full(R, 2, np.uint32)                            # every recording to the float32 member
    routes[0] = 3

    def routed_calls():
        out = list(routed_scan(bank, d, offs, lens, routes, n, sl)[0])
        out += routed_slide(bank, d, offs, lens, hop, AUTO, routes, n_slide)[0]
        s = outputs(gms, 9)
        bank.cmvn_inference_batch_device(mfcc.data_ptr(), 9, ptrs(s), None, routes=np.full(9, 2, np.uint32))
        return out + host(s)

    exact = routed_calls()
    assert same(exact[1][:n], own[1][0][:n]) and same(exact[2 * K + 1], own_c[1][:9])
    B = 16
    clips = torch.from_numpy(oracle.synth(31, 0, B)).cuda()
    tap = torch.full((B, gm.n_labels), -7.0, dtype=torch.float32, device="cuda")
    s_fast = torch.empty((B, gm.n_labels), dtype=torch.float32, device="cuda")
    gm.set_mode(pkg.MODE_FAST)
    gm.set_logits_tap(tap.data_ptr())
    try:
        gm.run_classifier_batch_device(clips.data_ptr(), B, s_fast.data_ptr())
        torch.cuda.synchronize()
        counts = (gm.fast_fallback_count(), gm.fast_exact_count())
        assert (tap.cpu().numpy() != -7.0).all()
        tap.fill_(-7.0)
        got = routed_calls()
        assert len(got) == len(exact) and all(same(a, b) for a, b in zip(got, exact))
        assert (tap.cpu().numpy() == -7.0).all(), "a routed bank call wrote a member's logits tap"
        assert gm.L.kws_get_mode(gm.h) == pkg.MODE_FAST and (gm.fast_fallback_count(), gm.fast_exact_count()) == counts
    finally:
        gm.set_logits_tap(None)
        gm.set_mode(pkg.MODE_EXACT)
