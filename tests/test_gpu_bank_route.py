"""Routed bank calls on the GPU (kws_bank_run_classifier_routed_device, kws_bank_run_classifier_ragged_routed_device, kws_bank_live_route,
kws_bank_slide_live_route; the contract is in include/kws/kws.h) on two banks of tests/test_gpu_bank.py / test_gpu_bank_windows.py: the four
49x40 models (matrix-core int8 at 64-byte rows, a class-2 int8 DS-CNN, two float graphs) and the l476 pair (matrix-core int8 at 16-byte
rows, plus float).  Every score buffer is filled with the bit pattern 0x7fc0dead before each call.  A routed (row, member) pair's row must
be the bits of the member's own entry point in KWS_MODE_EXACT and, on up to 64 clips, match the oracle (int8 bit-exact, float32 scores
within 1e-6); every other row must still hold the sentinel bits; `features` must be the unrouted call's bits.

No case is vacuous, as a condition on the inputs: wherever a call has more than one row and its routes are not one of the three kinds that
rule it out by their definition (all members; one member never named; only the last clip routed), every member has at least one routed and
one unrouted row -- asserted before the call; the three degenerate kinds assert what defines them instead."""
import os
import sys

import numpy as np
import pytest

from kws_testlib import MODELS, ROOT, OracleModel, bits, special_clips
from scan_testlib import oracle_scan, pack, speech

pytestmark = pytest.mark.gpu

F32_SCORE_TOL = 1e-6           # the project's bar for exact-mode float32 scores
SENTINEL_BITS = 0x7fc0dead     # a quiet NaN no kernel here produces
CLIP = 16000
KWS_NN_WAVES = 4               # clips per workgroup of the matrix-core network kernels (csrc/kws_nn_int8_dev.h)
DIRECT, SHARED = 1, 2
MFCC40 = ["cfg2_mfcc40_int8.kwsm", "cfg2_mfcc40_f32.kwsm", "cfg5_dscnn_mfcc40_int8.kwsm", "cfg5_dscnn_mfcc40_f32.kwsm"]
BANKS = {"49x40": MFCC40, "l476": ["l476_no_yes.kwsm", "l476_no_yes_f32.kwsm"]}
SIZES = [1, 2 * KWS_NN_WAVES + 1, 203]
KINDS = ["all", "never", "onehot", "random", "last"]
ORACLE_ROWS = 64


# ---- routes: pure host arithmetic ----------------------------------------------------------------------------------------------------
def make_routes(kind, B, K, seed=0):
    every = (1 << K) - 1
    if kind == "all":
        return np.full(B, every, np.uint32)
    if kind == "never":                      # member 1 is never named; the others by a seeded choice, never nobody
        rng = np.random.default_rng(seed)
        r = rng.integers(1, 1 << K, B).astype(np.uint32) & np.uint32(every & ~2)
        r[r == 0] = 1
        return r
    if kind == "onehot":
        return (np.uint32(1) << (np.arange(B) % K).astype(np.uint32)).astype(np.uint32)
    if kind == "random":                     # seeded masks, a fifth of them zero; rows 0 .. K - 1 make sure everybody is named and left out once
        rng = np.random.default_rng(seed)
        r = rng.integers(0, 1 << K, B).astype(np.uint32)
        r[rng.random(B) < 0.2] = 0
        if B > K:
            r[:K] = np.uint32(1) << np.arange(K).astype(np.uint32)
            r[K] = 0
        return r
    if kind == "last":
        r = np.zeros(B, np.uint32)
        r[B - 1] = 1 << (K - 1)
        return r
    raise ValueError(kind)


def routed(routes, k):
    return ((np.asarray(routes, np.uint32) >> np.uint32(k)) & 1).astype(bool)


def assert_not_vacuous(routes, K, what):
    for k in range(K):
        m = routed(routes, k)
        assert m.any() and not m.all(), (what, k)


def test_routes_of_every_case_meet_their_conditions():
    """the inputs of the GPU cases, checked as arithmetic (no device work): see the module docstring"""
    for K in (2, 4):
        for B in SIZES:
            for kind in KINDS:
                r = make_routes(kind, B, K, seed=B)
                assert r.shape == (B,) and (r < (1 << K)).all()
                if kind == "all":
                    assert all(routed(r, k).all() for k in range(K))
                elif kind == "never":
                    assert not routed(r, 1).any() and (r != 0).all()
                elif kind == "last":
                    assert int(np.count_nonzero(r)) == 1 and r[B - 1] == 1 << (K - 1)
                elif B > K:
                    assert_not_vacuous(r, K, (kind, B, K))
                    assert kind != "random" or (r == 0).any()


# ---- fixtures ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pkg():
    sys.path.insert(0, ROOT)
    import torch  # noqa: F401
    from __graft_entry__ import load_package
    return load_package()


@pytest.fixture(scope="module")
def banks(pkg, oracle):
    """bank name -> (Bank, [(product model, oracle model)]), created once per module"""
    models, made = {}, {}

    def get(name):
        if name not in made:
            for n in BANKS[name]:
                if n not in models:
                    models[n] = (pkg.Model(os.path.join(MODELS, n)), OracleModel(oracle, os.path.join(MODELS, n)))
            members = [models[n] for n in BANKS[name]]
            made[name] = (pkg.Bank([gm for gm, _ in members]), members)
        return made[name]

    yield get
    for bank, _ in made.values():
        bank.close()
    for gm, _ in models.values():
        gm.close()


@pytest.fixture(scope="module")
def clips(oracle):
    """[203][CLIP] int16: every special clip, then speech-like clips; computed once, never written"""
    sp = np.stack(list(special_clips().values()))
    pcm = np.concatenate([sp, oracle.synth(31, 0, max(SIZES) - sp.shape[0])])
    pcm.setflags(write=False)
    return pcm


@pytest.fixture(scope="module")
def own_rows(banks, clips):
    """bank name -> ([scores of each member's own kws_run_classifier_batch_device], features of the unrouted bank call) on all clips, once"""
    made = {}

    def get(name):
        import torch
        if name not in made:
            bank, members = banks(name)
            B = clips.shape[0]
            d = torch.from_numpy(clips.copy()).cuda()
            own = []
            for gm, _ in members:
                s = torch.empty((B, gm.n_labels), dtype=torch.float32, device="cuda")
                gm.run_classifier_batch_device(d.data_ptr(), B, s.data_ptr(), None)
                own.append(s)
            made[name] = (host(own), d)
        return made[name]

    return get


@pytest.fixture(scope="module")
def oracle_rows(banks, clips):
    """bank name -> [oracle scores of each member] on the first 64 clips, once"""
    made = {}

    def get(name):
        if name not in made:
            made[name] = [om.run_batch(clips[:ORACLE_ROWS]) for _, om in banks(name)[1]]
        return made[name]

    return get


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
    """rows of `mask`: the bits of `want`; every other row: the sentinel bits"""
    assert same(got[mask], want[mask]), what
    assert untouched(got[~mask]), what


def check_oracle(got, want, is_float, what):
    if not got.size:
        return
    if is_float:
        err = float(np.abs(got - want).max())
        print("%s: max |score - oracle| %.3g" % (what, err))
        assert err <= F32_SCORE_TOL, (what, err)
    else:
        assert same(got, want), what


# ---- clips ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", SIZES)
@pytest.mark.parametrize("name", list(BANKS))
def test_routed_clips_match_each_member_and_the_oracle(name, B, pkg, banks, clips, own_rows, oracle_rows):
    import torch
    bank, members = banks(name)
    gms, K = bank.members, len(members)
    own, d = own_rows(name)
    ref = oracle_rows(name)
    F = gms[0].n_features
    # the unrouted call: its features are the routed calls', its rows the members' own
    s0, f0 = outputs(gms, B + 2), sentinel(B + 2, F)
    bank.run_classifier_batch_device(d.data_ptr(), B, ptrs(s0), f0.data_ptr())
    s0, f0 = host(s0), host([f0])[0]
    assert all(same(s0[k][:B], own[k][:B]) and untouched(s0[k][B:]) for k in range(K)) and untouched(f0[B:])
    for kind in KINDS:
        routes = make_routes(kind, B, K, seed=B)
        if B > K and kind in ("onehot", "random"):
            assert_not_vacuous(routes, K, (name, B, kind))
        for with_features in (True, False):
            s, f = outputs(gms, B + 2), sentinel(B + 2, F)
            bank.run_classifier_routed_device(d.data_ptr(), B, routes, ptrs(s), f.data_ptr() if with_features else None)
            s, f = host(s), host([f])[0]
            assert same(f, f0) if with_features else untouched(f), (name, B, kind)
            for k, (gm, om) in enumerate(members):
                what = "%s / %s B %d %s" % (name, BANKS[name][k], B, kind)
                mask = np.concatenate([routed(routes, k), [False, False]])
                check_member(s[k], np.concatenate([own[k][:B], own[k][:2]]), mask, what)
                n = min(B, ORACLE_ROWS)
                check_oracle(s[k][:n][mask[:n]], ref[k][:n][mask[:n]], gm.is_float, what)
    # routes == None is the unrouted call
    s, f = outputs(gms, B + 2), sentinel(B + 2, F)
    bank.run_classifier_routed_device(d.data_ptr(), B, None, ptrs(s), f.data_ptr())
    s, f = host(s), host([f])[0]
    assert all(same(a, b) for a, b in zip(s, s0)) and same(f, f0)
    # a route bit at or above K: refused, nothing written
    bad = make_routes("onehot", B, K)
    bad[B - 1] |= 1 << K
    s = outputs(gms, B)
    with pytest.raises(pkg.KwsError) as e:
        bank.run_classifier_routed_device(d.data_ptr(), B, bad, ptrs(s), None)
    assert e.value.code == -20 and "clip %d" % (B - 1) in str(e.value) and all(untouched(t) for t in host(s))


def test_routed_clips_beyond_the_grid_cap(pkg, banks):
    """the l476 pair one tile above the matrix-core kernel's grid cap (n_cu x 4 workgroups of KWS_NN_WAVES clips): the list walk's stride
    loop.  One-hot routes with every third clip to both members; against the members' own calls (the oracle is too slow for this count)"""
    import torch
    bank, members = banks("l476")
    gms = bank.members
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    B = n_cu * 4 * KWS_NN_WAVES + 37
    d = torch.empty((B, CLIP), dtype=torch.int16, device="cuda")
    pkg.synth_clips_device(77, 0, B, CLIP, d.data_ptr())
    onehot = make_routes("onehot", B, 2)
    onehot[::3] = 3
    # those routes leave both lists under one pass of the capped grid; a second set sends all but twenty clips to member 0, so that its
    # list alone is longer than one pass and its waves take a second clip
    heavy = np.ones(B, np.uint32)
    heavy[::3] = 3
    heavy[100:120] = 2
    assert int(routed(heavy, 0).sum()) > n_cu * 4 * KWS_NN_WAVES and B > n_cu * 4 * KWS_NN_WAVES
    own = []
    for gm in gms:
        so = torch.empty((B, gm.n_labels), dtype=torch.float32, device="cuda")
        fo = torch.empty((B, gm.n_features), dtype=torch.float32, device="cuda")
        gm.run_classifier_batch_device(d.data_ptr(), B, so.data_ptr(), fo.data_ptr())
        own.append((so, fo))
    torch.cuda.synchronize()
    for routes in (onehot, heavy):
        assert_not_vacuous(routes, 2, "stride loop")
        s, f = outputs(gms, B + 1), sentinel(B + 1, gms[0].n_features)
        bank.run_classifier_routed_device(d.data_ptr(), B, routes, ptrs(s), f.data_ptr())
        torch.cuda.synchronize()
        for k, (so, fo) in enumerate(own):
            mask = torch.from_numpy(np.concatenate([routed(routes, k), [False]])).cuda()
            got = s[k].view(torch.int32)
            assert bool((got[:B][mask[:B]] == so.view(torch.int32)[mask[:B]]).all()), k
            assert bool((got[~mask] == SENTINEL_BITS).all()), k
            assert bool((f.view(torch.int32)[:B] == fo.view(torch.int32)).all()) and bool((f.view(torch.int32)[B:] == SENTINEL_BITS).all()), k


# ---- clips of their own lengths ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(BANKS))
def test_routed_ragged_matches_each_member_and_the_oracle(name, pkg, oracle, banks):
    """B = 67: 1-frame clips and full clips among lengths in between, at aligned offsets (read in place) and odd ones (staged)"""
    import torch
    from test_gpu_ragged import _compose
    bank, members = banks(name)
    gms, K = bank.members, len(members)
    B = 67
    rng = np.random.default_rng(67)
    lens = [640, CLIP, 640 + 319, 9001, CLIP, 5000, 640, 12345][:8] * 9
    lens = [int(x) for x in lens[:B]]
    lens[10:40] = [int(x) for x in rng.integers(640, CLIP + 1, 30)]
    assert lens.count(640) >= 3 and lens.count(CLIP) >= 3 and all(gms[0].window_frame_count(n) >= 1 for n in lens)
    pool = oracle.synth(88, 0, B, CLIP)
    cl = [pool[i][:n] for i, n in enumerate(lens)]
    buf = np.random.default_rng(9).integers(-32768, 32768, sum(lens) + 16 * B + 64, dtype=np.int16)
    offs, at = [], 0
    for i, c in enumerate(cl):
        at = (at + 7) // 8 * 8 + (i % 2) * (1 + 2 * (i % 4))       # even i: on a 16-byte boundary; odd i: an odd sample
        buf[at:at + c.size] = c
        offs.append(at)
        at += c.size
    assert [o % 8 == 0 for o in offs] == [i % 2 == 0 for i in range(B)]
    d = torch.from_numpy(buf).cuda()
    assert d.data_ptr() % 16 == 0
    offs, lens_a = np.array(offs, np.uint64), np.array(lens, np.uint64)
    F = gms[0].n_features
    routes = make_routes("random", B, K, seed=167)
    assert_not_vacuous(routes, K, (name, "ragged"))
    assert (routes == 0).any()
    s0, f0 = outputs(gms, B + 2), sentinel(B + 2, F)
    bank.run_classifier_ragged_device(d.data_ptr(), offs, lens_a, ptrs(s0), f0.data_ptr())
    f0 = host([f0])[0]
    s, f = outputs(gms, B + 2), sentinel(B + 2, F)
    bank.run_classifier_ragged_device(d.data_ptr(), offs, lens_a, ptrs(s), f.data_ptr(), routes=routes)
    s, f = host(s), host([f])[0]
    assert same(f, f0) and untouched(f[B:])
    for k, (gm, om) in enumerate(members):
        what = "%s / %s ragged" % (name, BANKS[name][k])
        so = sentinel(B + 2, gm.n_labels)
        gm.run_classifier_ragged_device(d.data_ptr(), offs, lens_a, so.data_ptr(), None, None)
        so = host([so])[0]
        mask = np.concatenate([routed(routes, k), [False, False]])
        check_member(s[k], so, mask, what)
        rows = [i for i in range(ORACLE_ROWS) if mask[i]]
        want = np.stack([_compose(oracle, om, cl[i])[2].reshape(-1) for i in rows])
        check_oracle(s[k][rows], want, gm.is_float, what)
    bad = routes.copy()
    bad[5] = 1 << K
    t = outputs(gms, B)
    with pytest.raises(pkg.KwsError) as e:
        bank.run_classifier_ragged_device(d.data_ptr(), offs, lens_a, ptrs(t), None, routes=bad)
    assert e.value.code == -20 and "clip 5" in str(e.value) and all(untouched(x) for x in host(t))


# ---- live continuous streams ---------------------------------------------------------------------------------------------------------
def stream_routes(K):
    """stream 0 -> member 0 only, 1 -> member 1 only, 2 -> both of them, 3 -> none, 4 -> all"""
    return np.array([1, 2, 3, 0, (1 << K) - 1], np.uint32)


class RoutedLive:
    """a routed bank session next to K single-model sessions fed the same pushes: a routed (stream, member) pair's rows of scores and
    raw_scores in bits against the member's own session, the sentinel everywhere else"""

    def __init__(self, bank, S, sl):
        self.gms = bank.members
        self.lv = bank.live_streams(S, sl)
        self.own = [gm.live_streams(S, sl) for gm in self.gms]
        self.route = np.full(S, (1 << len(self.gms)) - 1, np.uint32)
        self.rows = {}                                            # (stream, member) -> list of score rows, for the oracle
        self.counts = set()

    def set_route(self, streams, routes):
        self.lv.route(streams, routes)
        self.route[list(streams)] = routes

    def reset(self, streams):
        self.lv.reset(streams)
        for o in self.own:
            o.reset(streams)

    def push(self, entries, seed, skip_unneeded=False):
        import torch
        streams = [e[0] for e in entries]
        chunks = [np.asarray(e[1], np.int16) for e in entries]
        fin = [int(bool(e[2])) for e in entries]
        want = [self.lv.window_count(s, c.size, f) for s, c, f in zip(streams, chunks, fin)]
        self.counts |= set(want)
        n = sum(want)
        pcm, offs, lens = pack(chunks, seed=seed, max_gap=9)
        d = torch.from_numpy(pcm).cuda()
        needed = 0
        for s in streams:
            needed |= int(self.route[s])
        skip = {k for k in range(len(self.gms)) if skip_unneeded and not (needed >> k) & 1}
        sc, rw = outputs(self.gms, n + 3), outputs(self.gms, n + 3)
        nw = self.lv.push_device(d.data_ptr(), streams, offs, lens, ptrs(sc, skip), ptrs(rw, skip), finish=fin)
        assert [int(x) for x in nw] == want
        sc, rw = host(sc), host(rw)
        row_route = np.concatenate([np.repeat(self.route[streams], want), np.zeros(3, np.uint32)]) if streams else np.zeros(3, np.uint32)
        for k, gm in enumerate(self.gms):
            so, ro = sentinel(n + 3, gm.n_labels), sentinel(n + 3, gm.n_labels)
            nwo = self.own[k].push_device(d.data_ptr(), streams, offs, lens, so.data_ptr(), ro.data_ptr(), finish=fin)
            assert [int(x) for x in nwo] == want
            so, ro = host([so, ro])
            mask = routed(row_route, k)
            check_member(sc[k], so, mask, ("scores", k, streams))
            check_member(rw[k], ro, mask, ("raw_scores", k, streams))
            pos = 0
            for s, w in zip(streams, want):
                if (int(self.route[s]) >> k) & 1:
                    self.rows.setdefault((s, k), []).extend(sc[k][pos:pos + w])
                pos += w
        return want

    def close(self):
        self.lv.close()
        for o in self.own:
            o.close()


@pytest.mark.parametrize("name", list(BANKS))
def test_routed_live_pushes_match_the_members_own_sessions_and_the_oracle(name, pkg, oracle, banks):
    bank, members = banks(name)
    K = len(members)
    S, sl, g = 5, 4000, 320
    recs = [speech(oracle, 900 + s, 11 * sl + g + 5 + s) for s in range(S)]
    again = speech(oracle, 950, 7 * sl + g)                     # stream 3 after its reset
    routes = stream_routes(K)
    for k in range(K):                                           # every member has streams it serves and streams it does not
        assert routed(routes, k).any() and not routed(routes, k).all(), k
    chk = RoutedLive(bank, S, sl)
    try:
        chk.set_route(range(S), routes)
        pos = [0] * S

        def take(s, n, rec=None):
            rec = recs[s] if rec is None else rec
            c = rec[pos[s]:pos[s] + n]
            pos[s] += c.size
            return c
        chk.push([(s, take(s, 3 * sl), False) for s in range(S)], seed=1)                       # no window yet
        w = chk.push([(s, take(s, sl + g), False) for s in (0, 1, 2, 4)], seed=2)               # the first window of each
        assert w == [1, 1, 1, 1]
        w = chk.push([(s, take(s, 3 * sl), False) for s in (4, 0, 3, 2)], seed=3)
        assert w == [3, 3, 2, 3]
        # a stream that has been pushed to keeps its route: refused, and the pushes that follow return what they would have
        with pytest.raises(pkg.KwsError) as e:
            chk.lv.route([3, 0], [1, 2])
        assert e.value.code == -20
        # stream 1 finishes mid-way; stream 2 gets nothing new; members nobody here names are skipped with NULL buffers
        w = chk.push([(1, take(1, 17), True), (2, take(2, 0), False)], seed=4, skip_unneeded=True)
        assert w[1] == 0
        fed1 = pos[1]                                            # stream 1's recording ends here
        # a reset, then a new route: stream 3 (nobody so far) starts over for the last member alone
        chk.reset([3])
        chk.set_route([3], [1 << (K - 1)])
        pos[3] = 0
        chk.rows = {key: v for key, v in chk.rows.items() if key[0] != 3}
        chk.push([(3, take(3, 5 * sl + g, again), False), (0, take(0, sl - 1), False)], seed=5)
        chk.push([(0, take(0, recs[0].size), True), (2, take(2, recs[2].size), True), (3, take(3, again.size, again), True), (4, take(4, recs[4].size), True)], seed=6)
        assert {0, 1, 3} <= chk.counts
        # the oracle on one stream per member: its whole recording, window after window (int8 bit-exact, float32 within 1e-6)
        for k, (gm, om) in enumerate(members):
            s = k if k < 2 else 4
            rec = recs[s][:fed1] if s == 1 else recs[s]
            got = np.array(chk.rows[(s, k)], np.float32).reshape(-1, gm.n_labels)
            want = oracle_scan(om, rec, sl)
            assert got.shape == want.shape and got.shape[0] == (1 if s == 1 else 8), (name, k, got.shape, want.shape)
            check_oracle(got, want, gm.is_float, "%s / %s live stream %d" % (name, BANKS[name][k], s))
        got = np.array(chk.rows[(3, K - 1)], np.float32).reshape(-1, members[K - 1][0].n_labels)
        check_oracle(got, oracle_scan(members[K - 1][1], again, sl), members[K - 1][0].is_float, "%s stream 3 rerouted" % name)
        # a needed scores[k] that is NULL: refused, nothing changes
        import torch
        d = torch.from_numpy(recs[0]).cuda()
        sc = outputs(bank.members, 8)
        before = chk.lv.window_count(0, 5 * sl, False)
        with pytest.raises(pkg.KwsError) as e:
            chk.lv.push_device(d.data_ptr(), [0], [0], [5 * sl], ptrs(sc, skip={0}), None)
        assert e.value.code == -20 and chk.lv.window_count(0, 5 * sl, False) == before and all(untouched(t) for t in host(sc))
    finally:
        chk.close()


# ---- live one-shot windows -----------------------------------------------------------------------------------------------------------
def test_routed_live_one_shot_paths_cover_what_a_session_can_report(pkg, banks):
    """hop 1600 and hop 1000 between them run every path kws_bank_slide_live_path reports (host arithmetic at create)"""
    bank, _ = banks("l476")
    got = set()
    for hop in (1600, 1000):
        sess = bank.slide_streams(5, hop)
        got.add(sess.path)
        sess.close()
    assert got == {DIRECT, SHARED}


@pytest.mark.parametrize("hop", [1600, 1000])
@pytest.mark.parametrize("name", list(BANKS))
def test_routed_live_one_shot_matches_the_members_own_sessions(name, hop, pkg, oracle, banks):
    import torch
    bank, members = banks(name)
    gms, K = bank.members, len(members)
    S = 5
    recs = [speech(oracle, 1000 + s, CLIP + 7 * hop + 11 * s) for s in range(S)]
    pcm, offs, lens = pack(recs, seed=13)
    d = torch.from_numpy(pcm).cuda()
    route = stream_routes(K)
    shifted = np.array([2, 1, 0, (1 << K) - 1, 3], np.uint32)    # the routes after the change between two pushes
    for r in (route, shifted):
        for k in range(K):
            assert routed(r, k).any() and not routed(r, k).all(), k
    sess = bank.slide_streams(S, hop)
    own = [gm.slide_streams(S, hop) for gm in gms]
    try:
        assert all(o.path == sess.path for o in own)
        sess.route(range(S), route)
        pos = [0] * S
        plan = [([0, 1, 2, 3, 4], CLIP - 1), ([4, 2, 0, 1, 3], 1 + 2 * hop), ([1, 3], hop + 5), ("reroute", 0), ([3, 0, 2, 4, 1], 3 * hop), ([2, 4], 10 ** 6)]
        seen = 0
        for step, (streams, m) in enumerate(plan):
            if streams == "reroute":
                sess.route(range(S), shifted)
                route = shifted
                continue
            ln = [min(m, recs[s].size - pos[s]) for s in streams]
            of = [int(offs[s]) + pos[s] for s in streams]
            want = [sess.window_count(s, x) for s, x in zip(streams, ln)]
            n = sum(want)
            sc, ft = outputs(gms, n + 2), sentinel(n + 2, gms[0].n_features)
            nw = sess.push_device(d.data_ptr(), streams, of, ln, ptrs(sc), ft.data_ptr() if step % 2 == 0 else None)
            assert [int(x) for x in nw] == want, (name, hop, step)
            sc, ft = host(sc), host([ft])[0]
            row_route = np.concatenate([np.repeat(route[streams], want), np.zeros(2, np.uint32)])
            for k, gm in enumerate(gms):
                so, fo = sentinel(n + 2, gm.n_labels), sentinel(n + 2, gm.n_features)
                nwo = own[k].push_device(d.data_ptr(), streams, of, ln, so.data_ptr(), fo.data_ptr())
                assert [int(x) for x in nwo] == want
                so, fo = host([so, fo])
                check_member(sc[k], so, routed(row_route, k), (name, hop, step, k))
                assert same(ft, fo) if step % 2 == 0 else untouched(ft), (name, hop, step, k)
            for s, x in zip(streams, ln):
                pos[s] += x
            seen += n
        assert seen >= 20
        with pytest.raises(pkg.KwsError) as e:
            sess.route([0], [1 << K])
        assert e.value.code == -20
    finally:
        sess.close()
        for o in own:
            o.close()
