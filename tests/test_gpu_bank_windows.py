"""The banks' window pipelines: kws_bank_scan_recordings_device, kws_bank_live_*, kws_bank_slide_live_* and
kws_bank_run_classifier_ragged_device on the banks of tests/test_gpu_bank.py (the 49x13 bank with one more member of five labels, so that
label counts differ within a bank).  Every member's rows in bits against that member's own entry point in KWS_MODE_EXACT -- for the live
sessions push by push against K single-model sessions fed the same pushes -- and, on the 49x13 and MFE banks, against the oracle (int8
bit-exact, float32 within 1e-6); the shared features in bits; rows beyond a call's windows and a skipped member's buffer untouched; the
members' mode, fast counters and logits tap untouched."""
import os
import sys

import numpy as np
import pytest

from kws_testlib import MODELS, ROOT, OracleModel, bits, synth_model_blob
from continuous_geometry import GRID
from live_testlib import run_random_chunking
from scan_testlib import moving_average, oracle_scan, pack, speech
from slide_live_testlib import AUTO, SHARED, auto_path, edge_lengths, paths_for
from slide_testlib import cut_windows
from test_gpu_bank import BANKS as BASE_BANKS, _blob

pytestmark = pytest.mark.gpu

F32_SCORE_TOL = 1e-6           # the project's bar for exact-mode float32 scores
SENTINEL = -7.0
CLIP = 16000
SYNTH13_L5 = dict(seed=8, blocks=((12, 5, 2), (6, 3, 2)), n_labels=5)
BANKS = {name: list(members) for name, (members, _) in BASE_BANKS.items()}
BANKS["49x13"].append("synth13_l5")
ORACLE_BANKS = ("49x13", "mfe")
# the scan's slicing per bank: 4000 samples, and for the stride-10 ms front end (which the stream API refuses at 4000) the second slicing of
# tests/continuous_geometry.py
SLICES = {"49x13": 4000, "49x40": 4000, "mfe": 4000, "stride10": GRID["stride10"][1][1]}


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
    tmp = tmp_path_factory.mktemp("bank_windows")

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


def outputs(gms, rows):
    import torch
    return [torch.full((rows, gm.n_labels), SENTINEL, dtype=torch.float32, device="cuda") for gm in gms]


def ptrs(tensors, skip=()):
    return [None if k in skip else t.data_ptr() for k, t in enumerate(tensors)]


def host(tensors):
    import torch
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in tensors]


def same(a, b):
    return a.shape == b.shape and bool((bits(a) == bits(b)).all())


def check_oracle(got, want, is_float, what):
    if is_float:
        err = float(np.abs(got - want).max()) if got.size else 0.0
        print("%s: max |score - oracle| %.3g" % (what, err))
        assert err <= F32_SCORE_TOL, (what, err)
    else:
        assert same(got, want), what


def grow_of(om):
    return int(np.float32(om.cfg.frame_length) * np.float32(om.cfg.sampling_frequency))


# ---- the scan ------------------------------------------------------------------------------------------------------------------
def bank_scan(bank, d, offs, lens, n, slice_samples, raw=True, skip=()):
    gms = bank.members
    s, r = outputs(gms, n + 2), outputs(gms, n + 2)
    bank.scan_recordings_device(d.data_ptr(), offs, lens, ptrs(s, skip), ptrs(r, skip) if raw else None, slice_samples=slice_samples)
    return host(s), host(r)


def own_scan(gm, d, offs, lens, n, slice_samples):
    s, r = outputs([gm], max(n, 1)), outputs([gm], max(n, 1))
    gm.scan_recordings_device(d.data_ptr(), offs, lens, s[0].data_ptr(), r[0].data_ptr(), slice_samples=slice_samples)
    return host(s)[0][:n], host(r)[0][:n]


@pytest.mark.parametrize("name", list(BANKS))
def test_bank_scan_matches_each_member_and_the_oracle(name, pkg, oracle, banks):
    """five recordings around the first window's edges (0 windows, 1 window, a trailing partial slice, 3 and 7 windows at the shipped
    geometry) in one call at odd offsets: with and without raw_scores, with one member skipped"""
    import torch
    bank, members = banks(name)
    gms = bank.members
    sl = SLICES[name]
    k1 = next(k for k in range(1, 64) if gms[0].scan_window_count(k * sl, sl))         # slices up to the first window: 4 at 4000 samples
    lengths = [k1 * sl - 1, k1 * sl, k1 * sl + sl - 1, (k1 + 2) * sl, (k1 + 6) * sl]
    assert sl != 4000 or lengths == [15999, 16000, 16000 + 3999, 24000, 40000]
    recs = [speech(oracle, 500 + i, n) for i, n in enumerate(lengths)]
    pcm, offs, lens = pack(recs, seed=11)
    assert sum(int(o) % 2 for o in offs) >= 3                     # most recordings start on an odd sample
    W = [gms[0].scan_window_count(int(x), sl) for x in lens]
    assert all([gm.scan_window_count(int(x), sl) for x in lens] == W for gm in gms)
    assert W == [0, 1, 1, 3, 7]
    n = sum(W)
    if name == "49x13":
        assert len({gm.n_labels for gm in gms}) > 1
    if name == "stride10":
        with pytest.raises(pkg.KwsError) as e:                   # the stream API refuses 4000 for this front end: so does the bank, with its code
            bank_scan(bank, torch.from_numpy(pcm).cuda(), offs, lens, n, 4000)
        assert e.value.code == -5
    d = torch.from_numpy(pcm).cuda()
    s, r = bank_scan(bank, d, offs, lens, n, sl)
    s2, r2 = bank_scan(bank, d, offs, lens, n, sl, raw=False)
    skip = len(gms) - 1
    s3, r3 = bank_scan(bank, d, offs, lens, n, sl, skip={skip})
    cut = np.cumsum([0] + W)
    for k, (gm, om) in enumerate(members):
        what = "%s / %s" % (name, BANKS[name][k])
        s_own, r_own = own_scan(gm, d, offs, lens, n, sl)
        assert same(s[k][:n], s_own) and same(r[k][:n], r_own), what
        assert (s[k][n:] == SENTINEL).all() and (r[k][n:] == SENTINEL).all(), what
        assert same(s2[k][:n], s_own) and (s2[k][n:] == SENTINEL).all() and (r2[k] == SENTINEL).all(), what
        if k == skip:
            assert (s3[k] == SENTINEL).all() and (r3[k] == SENTINEL).all(), what
        else:
            assert same(s3[k], s[k]) and same(r3[k], r[k]), what
        if name in ORACLE_BANKS:
            for i, rec in enumerate(recs):
                want = oracle_scan(om, rec, sl)                          # (the oracle's scores: behind its moving average)
                assert want.shape[0] == W[i], (what, i)
                check_oracle(s[k][cut[i]:cut[i + 1]], want, gm.is_float, what + " recording %d" % i)
                assert same(moving_average(r[k][cut[i]:cut[i + 1]]), s[k][cut[i]:cut[i + 1]]), (what, i)
    with pytest.raises(pkg.KwsError) as e:
        bank.scan_recordings_device(d.data_ptr(), offs, lens, [None] * len(gms), None, slice_samples=sl)
    assert e.value.code == -20


def test_bank_scan_across_a_gather_chunk(pkg, banks):
    """one recording of 26 400 windows on the 49x13 bank: more than one chunk of gathered windows (kws_window_chunk(637, .) = 26 337), so the
    second chunk's rows go to row0 > 0 of buffers whose label counts differ; against the members' own scans"""
    import torch
    bank, members = banks("49x13")
    gms = bank.members
    n_slices = 26400 + 3
    total = 4000 * n_slices
    n_clips = (total + 1 + CLIP - 1) // CLIP
    big = torch.empty(n_clips * CLIP + 16, dtype=torch.int16, device="cuda")
    pkg.synth_clips_device(91, 0, n_clips, CLIP, big.data_ptr())
    torch.cuda.synchronize()
    offs, lens = np.array([1], np.uint64), np.array([total], np.uint64)               # (one sample in: an odd offset)
    n = gms[0].scan_window_count(total, 4000)
    assert n == 26400 > 26337 and len({gm.n_labels for gm in gms}) > 1
    s, r = outputs(gms, n + 1), outputs(gms, n + 1)
    bank.scan_recordings_device(big.data_ptr(), offs, lens, ptrs(s), ptrs(r), slice_samples=4000)
    torch.cuda.synchronize()
    for k, gm in enumerate(gms):
        so, ro = outputs([gm], n)[0], outputs([gm], n)[0]
        gm.scan_recordings_device(big.data_ptr(), offs, lens, so.data_ptr(), ro.data_ptr(), slice_samples=4000)
        torch.cuda.synchronize()
        assert bool((s[k][:n].view(torch.int32) == so.view(torch.int32)).all()) and bool((r[k][:n].view(torch.int32) == ro.view(torch.int32)).all()), k
        assert bool((s[k][n:] == SENTINEL).all()) and bool((r[k][n:] == SENTINEL).all()), k
        assert bool((so[26337:] != SENTINEL).all())


# ---- live continuous streams ---------------------------------------------------------------------------------------------------
class BankLiveCheck:
    """A bank session next to K single-model sessions fed the same pushes: every push's counts against kws_bank_live_window_count and the
    members' own pushes, every member's rows (scores and raw scores) in bits against its own session's and against the next windows of
    the bank scan of the stream's recording, nothing written past the push's windows.  push(entries) has LiveCheck's shape, so
    live_testlib.run_random_chunking drives it."""

    def __init__(self, bank, n_streams, slice_samples):
        self.bank, self.gms = bank, bank.members
        self.lv = bank.live_streams(n_streams, slice_samples)
        self.own = [gm.live_streams(n_streams, slice_samples) for gm in self.gms]
        self.ref, self.got, self.pushes, self.windows = {}, {}, 0, 0

    def start(self, s, ref):
        """ref: per member (scores, raw) of the bank scan of the recording stream s is about to receive"""
        self.ref[s], self.got[s] = ref, 0

    def reset(self, streams):
        self.lv.reset(streams)
        for o in self.own:
            o.reset(streams)

    def push(self, entries, seed=None):
        streams = [e[0] for e in entries]
        chunks = [np.asarray(e[1], np.int16) for e in entries]
        fin = [int(bool(e[2])) for e in entries]
        import torch
        want = [self.lv.window_count(s, c.size, f) for s, c, f in zip(streams, chunks, fin)]
        n = sum(want)
        pcm, offs, lens = pack(chunks, seed=self.pushes if seed is None else seed, max_gap=9)
        d = torch.from_numpy(pcm).cuda()
        sc, rw = outputs(self.gms, n + 3), outputs(self.gms, n + 3)
        nw = self.lv.push_device(d.data_ptr(), streams, offs, lens, ptrs(sc), ptrs(rw), finish=fin)
        self.pushes += 1
        self.windows += n
        assert [int(x) for x in nw] == want, (self.pushes, list(nw), want)
        sc, rw = host(sc), host(rw)
        for k, gm in enumerate(self.gms):
            so, ro = outputs([gm], n + 3)[0], outputs([gm], n + 3)[0]
            assert [self.own[k].window_count(s, c.size, f) for s, c, f in zip(streams, chunks, fin)] == want, (self.pushes, k)
            nwo = self.own[k].push_device(d.data_ptr(), streams, offs, lens, so.data_ptr(), ro.data_ptr(), finish=fin)
            assert [int(x) for x in nwo] == want, (self.pushes, k)
            so, ro = host([so, ro])
            assert same(sc[k], so) and same(rw[k], ro), (self.pushes, k)                    # (sentinel rows behind the windows included)
            assert (sc[k][n:] == SENTINEL).all() and (rw[k][n:] == SENTINEL).all(), (self.pushes, k)
            pos = 0
            for s, w in zip(streams, want):
                g = self.got[s]
                assert same(sc[k][pos:pos + w], self.ref[s][k][0][g:g + w]) and same(rw[k][pos:pos + w], self.ref[s][k][1][g:g + w]), (self.pushes, k, s, g, w)
                pos += w
        for s, w, f in zip(streams, want, fin):
            self.got[s] += w
            if f:
                assert self.got[s] == self.ref[s][0][0].shape[0], (self.pushes, s, self.got[s])
        return nw

    def close(self):
        self.lv.close()
        for o in self.own:
            o.close()


def scan_refs(bank, recs, slice_samples):
    """per recording, per member: (scores, raw) rows of one bank scan (which test_bank_scan holds to the members' own scans)"""
    import torch
    gms = bank.members
    pcm, offs, lens = pack(recs, seed=21)
    W = [gms[0].scan_window_count(int(x), slice_samples) for x in lens]
    n = sum(W)
    s, r = bank_scan(bank, torch.from_numpy(pcm).cuda(), offs, lens, n, slice_samples)
    cut = np.cumsum([0] + W)
    return [[(s[k][cut[i]:cut[i + 1]], r[k][cut[i]:cut[i + 1]]) for k in range(len(gms))] for i in range(len(recs))]


@pytest.mark.parametrize("name", list(BANKS))
def test_bank_live_pushes_match_k_sessions_and_the_bank_scan(name, pkg, oracle, banks):
    """S = 5: pushes of 0, 1, slice - 1, slice, slice + grow - 1 and slice + grow samples, finishes (one by a zero-length push), a reset of
    two streams mid-sequence, then every stream reused for a recording in random packets to random subsets"""
    bank, members = banks(name)
    sl, g = SLICES[name], grow_of(members[0][1])
    S = 5
    first = [speech(oracle, 600 + i, n) for i, n in enumerate([8 * sl + g, 7 * sl + 3, 6 * sl + g - 1, 9 * sl, 5 * sl + g + 1])]
    second = [speech(oracle, 620 + i, n) for i, n in enumerate([30011, 0, 47000, 16000 + 3999, 24000 + g])]
    ref1, ref2 = scan_refs(bank, first, sl), scan_refs(bank, second, sl)
    chk = BankLiveCheck(bank, S, sl)
    try:
        pos = [0] * S
        for s in range(S):
            chk.start(s, ref1[s])

        def take(s, n):
            c = first[s][pos[s]:pos[s] + n]
            pos[s] += c.size
            return c
        for step, n in enumerate([0, 1, sl - 1, sl, sl + g - 1, sl + g]):
            chk.push([(s, take(s, n), False) for s in range(S) if (s + step) % 4 != 3])
        # a reset of two streams mid-sequence: they start over, on their recordings from the first sample
        chk.reset([1, 3])
        for s in (1, 3):
            pos[s] = 0
            chk.start(s, ref1[s])
        chk.push([(s, take(s, 2 * sl + 17), False) for s in (3, 1, 4)])
        # everything that is left; streams 0 and 2 finish with their last samples, the others by a zero-length push
        chk.push([(s, take(s, first[s].size), s in (0, 2)) for s in range(S)])
        chk.push([(s, first[s][:0], True) for s in (4, 1, 3)])
        assert all(chk.got[s] == ref1[s][0][0].shape[0] for s in range(S)) and chk.windows >= 15
        # finished streams reused
        for s in range(S):
            chk.start(s, ref2[s])
        run_random_chunking(chk, second, np.random.default_rng(77))
        assert all(chk.got[s] == ref2[s][0][0].shape[0] for s in range(S))
        # a NULL scores[k] is refused and changes nothing: the next push still returns the scan's rows
        import torch
        chk.start(0, ref1[0])
        d = torch.from_numpy(first[0]).cuda()
        sc = outputs(bank.members, 8)
        before = chk.lv.window_count(0, 5 * sl, False)
        with pytest.raises(pkg.KwsError) as e:
            chk.lv.push_device(d.data_ptr(), [0], [0], [5 * sl], ptrs(sc, skip={0}), None)
        assert e.value.code == -20 and chk.lv.window_count(0, 5 * sl, False) == before and all((t == SENTINEL).all() for t in host(sc))
        chk.push([(0, first[0], True)])
    finally:
        chk.close()


# ---- live one-shot windows -----------------------------------------------------------------------------------------------------
def bank_slide(bank, d, offs, lens, hop, n, flags=AUTO):
    import torch
    gms = bank.members
    s = outputs(gms, n + 2)
    f = torch.full((n + 2, gms[0].n_features), SENTINEL, dtype=torch.float32, device="cuda")
    bank.slide_recordings_device(d.data_ptr(), offs, lens, hop, ptrs(s), f.data_ptr(), flags=flags)
    return host(s), host([f])[0]


@pytest.mark.parametrize("hop", [1600, 1000])
@pytest.mark.parametrize("name", list(BANKS))
def test_bank_slide_live_matches_k_sessions_and_the_bank_slide(name, hop, pkg, oracle, banks):
    """eight streams of lengths around every edge of the window count, random packets to random subsets, on every path the hop is served
    on: scores and features of every push in bits against each member's own session and against kws_bank_slide_recordings_device on the
    stream's whole recording (so DIRECT and SHARED are bit-identical to each other)"""
    import torch
    bank, members = banks(name)
    gms = bank.members
    gm0 = gms[0]
    pre = 0 if name == "mfe" else 1
    recs = [speech(oracle, 700 + i, n) for i, n in enumerate(edge_lengths(CLIP, hop))]
    S = len(recs)
    pcm, offs, lens = pack(recs, seed=3)
    d = torch.from_numpy(pcm).cuda()
    W = [gm0.slide_window_count(int(x), hop) for x in lens]
    assert W[:6] == [0, 0, 1, 1, 1, 2]
    n_all = sum(W)
    ref_s, ref_f = bank_slide(bank, d, offs, lens, hop, n_all)
    cut = np.cumsum([0] + W)
    if name in ORACLE_BANKS:
        windows, Wc = cut_windows(recs, CLIP, hop)
        assert Wc == W
        for k, (gm, om) in enumerate(members):
            so, fo, _ = om.run_batch(windows, want_features=True)
            assert same(ref_f[:n_all], fo), (name, hop, k)
            check_oracle(ref_s[k][:n_all], so, gm.is_float, "%s / %s hop %d" % (name, BANKS[name][k], hop))
    flags_list = paths_for(gm0, hop, pre)
    assert (SHARED in flags_list) == (hop == 1600)
    if SHARED not in flags_list:
        with pytest.raises(pkg.KwsError) as e:
            bank.slide_streams(S, hop, SHARED)
        assert e.value.code == -20
    for q, flags in enumerate(flags_list):
        sess = bank.slide_streams(S, hop, flags)
        own = [gm.slide_streams(S, hop, flags) for gm in gms]
        try:
            assert sess.path == (auto_path(gm0, hop, pre) if flags == AUTO else flags) and all(o.path == sess.path for o in own)
            rng = np.random.default_rng(1000 * q + hop)
            pos, got, pushes = [0] * S, [0] * S, 0
            while any(pos[s] < recs[s].size for s in range(S)):
                entries = []
                for s in rng.permutation(S):
                    if rng.random() > 0.6:
                        continue
                    kind = rng.integers(0, 4)
                    m = int(rng.integers(0, 5)) if kind == 0 else int(rng.integers(1, 401)) if kind == 1 else int(rng.integers(1, CLIP * 3 // 2))
                    entries.append((int(s), min(m, recs[s].size - pos[s])))
                st = [s for s, _ in entries]
                ln = [m for _, m in entries]
                of = [int(offs[s]) + pos[s] for s in st]
                want = [sess.window_count(s, m) for s, m in entries]
                n = sum(want)
                skip = {len(gms) - 1} if pushes % 3 == 2 else set()                  # every third push without the last member
                sc = outputs(gms, n + 2)
                ft = torch.full((n + 2, gm0.n_features), SENTINEL, dtype=torch.float32, device="cuda")
                nw = sess.push_device(d.data_ptr(), st, of, ln, ptrs(sc, skip), ft.data_ptr() if pushes % 2 == 0 else None)
                assert [int(x) for x in nw] == want, (name, hop, flags, pushes)
                sc, ft = host(sc), host([ft])[0]
                for k, gm in enumerate(gms):
                    so = outputs([gm], n + 2)[0]
                    fo = torch.full((n + 2, gm.n_features), SENTINEL, dtype=torch.float32, device="cuda")
                    nwo = own[k].push_device(d.data_ptr(), st, of, ln, so.data_ptr(), fo.data_ptr())
                    assert [int(x) for x in nwo] == want
                    so, fo = host([so, fo])
                    if k in skip:
                        assert (sc[k] == SENTINEL).all(), (name, hop, flags, pushes, k)
                    else:
                        assert same(sc[k], so), (name, hop, flags, pushes, k)
                    if pushes % 2 == 0:
                        assert same(ft, fo), (name, hop, flags, pushes, k)
                    else:
                        assert (ft == SENTINEL).all()
                row = 0
                for (s, m), w in zip(entries, want):
                    a = cut[s] + got[s]
                    for k in range(len(gms)):
                        assert k in skip or same(sc[k][row:row + w], ref_s[k][a:a + w]), (name, hop, flags, pushes, k, s)
                    assert pushes % 2 or same(ft[row:row + w], ref_f[a:a + w]), (name, hop, flags, pushes, s)
                    row += w
                    pos[s] += m
                    got[s] += w
                pushes += 1
            assert got == W and pushes >= 3
        finally:
            sess.close()
            for o in own:
                o.close()


# ---- clips of their own lengths ------------------------------------------------------------------------------------------------
def length_range(gm):
    """the shortest and the longest clip the ragged call accepts: 1 .. n_frames frames"""
    lo = next(n for n in range(1, CLIP) if gm.window_frame_count(n) >= 1)
    hi = CLIP
    while gm.window_frame_count(hi + 1) <= gm.n_frames:
        hi += 1
    return lo, hi


@pytest.mark.parametrize("name", list(BANKS))
def test_bank_ragged_matches_each_member_and_the_batch_call(name, pkg, oracle, banks):
    """lengths at both ends of the accepted range, a full-length clip, lengths in between, at aligned and unaligned offsets: the tuned
    route (49x13, 49x40) and the grouped route (mfe, stride10)"""
    import torch
    bank, members = banks(name)
    gms = bank.members
    gm0 = gms[0]
    lo, hi = length_range(gm0)
    assert gm0.window_frame_count(lo - 1) == 0 and gm0.window_frame_count(hi + 1) == gm0.n_frames + 1
    lens = [lo, hi, CLIP, lo + 1, hi - 1, 9001, 5000, CLIP, lo, 12345]
    FULL = [2, 7]                                                # the full-length clips: one aligned, one not
    pool = oracle.synth(88, 0, len(lens), hi)
    clips = [pool[i][:n] for i, n in enumerate(lens)]
    # clip i starts on a 16-byte boundary for even i and off it (an odd sample) for odd i
    buf = np.random.default_rng(9).integers(-32768, 32768, sum(lens) + 16 * len(lens) + 64, dtype=np.int16)
    offs, at = [], 0
    for i, c in enumerate(clips):
        at = (at + 7) // 8 * 8 + (i % 2) * (1 + 2 * (i % 4))
        buf[at:at + c.size] = c
        offs.append(at)
        at += c.size
    assert [o % 8 == 0 for o in offs] == [i % 2 == 0 for i in range(len(lens))]
    d = torch.from_numpy(buf).cuda()
    assert d.data_ptr() % 16 == 0
    B, F = len(lens), gm0.n_features
    offs, lens_a = np.array(offs, np.uint64), np.array(lens, np.uint64)

    def call(skip=(), want_features=True):
        s = outputs(gms, B + 2)
        f = torch.full((B + 2, F), SENTINEL, dtype=torch.float32, device="cuda")
        bank.run_classifier_ragged_device(d.data_ptr(), offs, lens_a, ptrs(s, skip), f.data_ptr() if want_features else None)
        return host(s), host([f])[0]
    s, f = call()
    s2, f2 = call(want_features=False)
    s3, f3 = call(skip={0})
    assert (f[B:] == SENTINEL).all() and (f2 == SENTINEL).all() and same(f3, f)
    cols = F // gm0.n_frames
    for i, n in enumerate(lens):
        used = gm0.window_frame_count(n) * cols
        assert (bits(f[i][used:]) == 0).all(), (name, i)                 # +0.0f behind the frames that fit
    full = torch.from_numpy(np.stack([clips[i] for i in FULL])).cuda()
    sb = outputs(gms, 2)
    fb = torch.empty((2, F), dtype=torch.float32, device="cuda")
    bank.run_classifier_batch_device(full.data_ptr(), 2, ptrs(sb), fb.data_ptr())
    sb, fb = host(sb), host([fb])[0]
    assert same(f[FULL], fb), name
    for k, gm in enumerate(gms):
        so = outputs([gm], B)[0]
        fo = torch.empty((B, F), dtype=torch.float32, device="cuda")
        gm.run_classifier_ragged_device(d.data_ptr(), offs, lens_a, so.data_ptr(), fo.data_ptr())
        so, fo = host([so, fo])
        assert same(s[k][:B], so) and (s[k][B:] == SENTINEL).all() and same(f[:B], fo), (name, k)
        assert same(s2[k], s[k]), (name, k)
        assert (s3[k] == SENTINEL).all() if k == 0 else same(s3[k], s[k]), (name, k)
        assert same(s[k][FULL], sb[k]), (name, k)
    for bad in ([lo - 1], [hi + 1]):
        t = outputs(gms, 1)
        with pytest.raises(pkg.KwsError) as e:
            bank.run_classifier_ragged_device(d.data_ptr(), [0], bad, ptrs(t), None)
        assert e.value.code == -20 and all((x == SENTINEL).all() for x in host(t))
    with pytest.raises(pkg.KwsError) as e:
        bank.run_classifier_ragged_device(d.data_ptr(), offs, lens_a, [None] * len(gms), None)
    assert e.value.code == -20


# ---- the members stay as they were ------------------------------------------------------------------------------------------------
def test_bank_window_calls_leave_the_members_untouched(pkg, oracle, banks):
    """the float32 member in KWS_MODE_FAST with a logits tap and counts from a fast call of its own: after bank calls in all four forms its
    mode, kws_fast_fallback_count, kws_fast_exact_count and tap are what they were, the bank wrote the exact bits, and the member's own
    exact call gives the bits it gave before"""
    import torch
    bank, members = banks("49x13")
    gms = bank.members
    gm = gms[1]
    assert gm.is_float
    sl, hop = 4000, 1600
    recs = [speech(oracle, 800 + i, n) for i, n in enumerate([24000, 40000 + 17])]
    pcm, offs, lens = pack(recs, seed=5)
    d = torch.from_numpy(pcm).cuda()
    n = sum(gm.scan_window_count(int(x), sl) for x in lens)
    nw_slide = sum(gm.slide_window_count(int(x), hop) for x in lens)
    rag_lens = np.array([9001, 16000], np.uint64)

    def bank_calls():
        out = list(bank_scan(bank, d, offs, lens, n, sl)[0])
        lv = bank.live_streams(2, sl)
        sc = outputs(gms, n + 2)
        nw = lv.push_device(d.data_ptr(), [0, 1], offs, lens, ptrs(sc), None, finish=[1, 1])
        assert int(nw.sum()) == n
        out += host(sc)
        lv.close()
        ss = bank.slide_streams(2, hop)
        sc = outputs(gms, nw_slide + 2)
        nw = ss.push_device(d.data_ptr(), [0, 1], offs, lens, ptrs(sc))
        assert int(nw.sum()) == nw_slide
        out += host(sc)
        ss.close()
        sc = outputs(gms, 2)
        bank.run_classifier_ragged_device(d.data_ptr(), offs, rag_lens, ptrs(sc))
        return out + host(sc)

    own_exact = own_scan(gm, d, offs, lens, n, sl)
    exact = bank_calls()
    B = 16
    clips = torch.from_numpy(oracle.synth(31, 0, B)).cuda()
    tap = torch.full((B, gm.n_labels), SENTINEL, dtype=torch.float32, device="cuda")
    s_fast = torch.empty((B, gm.n_labels), dtype=torch.float32, device="cuda")
    gm.set_mode(pkg.MODE_FAST)
    gm.set_logits_tap(tap.data_ptr())
    try:
        gm.run_classifier_batch_device(clips.data_ptr(), B, s_fast.data_ptr())
        torch.cuda.synchronize()
        counts = (gm.fast_fallback_count(), gm.fast_exact_count())
        assert (tap.cpu().numpy() != SENTINEL).all()
        tap.fill_(SENTINEL)
        got = bank_calls()
        assert len(got) == len(exact) and all(same(a, b) for a, b in zip(got, exact))
        assert (tap.cpu().numpy() == SENTINEL).all(), "a bank call wrote a member's logits tap"
        assert gm.L.kws_get_mode(gm.h) == pkg.MODE_FAST and (gm.fast_fallback_count(), gm.fast_exact_count()) == counts
    finally:
        gm.set_logits_tap(None)
        gm.set_mode(pkg.MODE_EXACT)
    again = own_scan(gm, d, offs, lens, n, sl)
    assert same(again[0], own_exact[0]) and same(again[1], own_exact[1])
