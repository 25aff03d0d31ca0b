"""kws_live_*: live streams in continuous mode, pushed audio of any length to any subset of streams.  Every push is checked on the spot
(live_testlib.LiveCheck): its window counts against kws_live_window_count, its windows bitwise against the next windows of
kws_scan_recordings_device on each stream's whole recording, nothing written past them.  The scan itself is held to the continuous oracle
here too, on the concatenations."""
import os

import numpy as np
import pytest

from kws_testlib import MODELS, OracleModel, bits
from live_testlib import SENTINEL, LiveCheck, run_random_chunking, scan_windows
from scan_testlib import SLICE, oracle_scan, recordings, speech
from test_gpu_scan import EXACT_MODELS, FAST_SCORE_TOL, check_exact, model_path, pkg  # noqa: F401  (pkg: the fixture)

pytestmark = pytest.mark.gpu

G = 320                                                            # the shipped models' frame length in samples: the look-ahead's reach
# 16 recordings of scan_testlib.recordings: empty, 1 sample, edge lengths around the first window and its look-ahead sample, 60 s,
# speech, digital silence, DC, audio that goes silent mid-recording
RANDOM_SET = [0, 1, 3, 4, 5, 6, 7, 8, 9, 10, 12, 13, 14, 28, 29, 31]


@pytest.fixture(scope="module")
def recs(oracle):
    return recordings(oracle)


@pytest.mark.parametrize("name", EXACT_MODELS)
def test_live_random_chunkings_match_the_scan(name, pkg, oracle, recs, tmp_path):
    """16 streams in seeded random packets (1 sample to 3 s) to random subsets, every stream finished: per stream the concatenated scores
    and raw scores are bitwise the scan's of the whole recording (and every prefix before the finish is the scan's first windows), and
    they match the oracle under test_gpu_scan's rules"""
    path = model_path(name, tmp_path)
    gm, om = pkg.Model(path), OracleModel(oracle, path)
    sub = [recs[i] for i in RANDOM_SET]
    ref = scan_windows(gm, sub)
    chk = LiveCheck(gm, len(sub))
    for i in range(len(sub)):
        chk.start(i, ref[i])
    run_random_chunking(chk, sub, np.random.default_rng(101 + EXACT_MODELS.index(name)))
    got = [chk.result(i) for i in range(len(sub))]
    for i in range(len(sub)):
        assert (bits(got[i][0]) == bits(ref[i][0])).all() and (bits(got[i][1]) == bits(ref[i][1])).all(), i
    W = [g[0].shape[0] for g in got]
    starts = np.concatenate([[0], np.cumsum(W)]).astype(np.int64)
    check_exact(om, sub, W, starts, np.concatenate([g[0] for g in got]), np.concatenate([g[1] for g in got]), gm.is_float)
    assert chk.pushes > 40
    chk.close()
    gm.close()


def test_live_boundaries(pkg, oracle):
    """packets that end on a slice edge; one sample before, on and after a look-ahead sample (which then arrives alone); one sample at a
    time across a slice edge and a look-ahead sample; a push that completes no window; a finish by a zero-length push; a finish of a
    stream that never reached a window"""
    gm = pkg.Model(os.path.join(MODELS, "l476_no_yes.kwsm"))
    n = 40000 + G
    rec = [speech(oracle, 300 + i, n) for i in range(6)]
    short = speech(oracle, 310, 12000 + 77)
    ref = scan_windows(gm, rec + [short])
    chk = LiveCheck(gm, 7)
    for i in range(7):
        chk.start(i, ref[i])
    # a push to three fresh streams that completes no window: nothing written, every count 0
    nw = chk.push([(0, rec[0][:100], False), (1, rec[1][:100], False), (6, short[:100], False)])
    assert list(nw) == [0, 0, 0]
    la = lambda k: (k + 1) * SLICE + G - 1                         # the look-ahead sample of slice k >= 1
    cuts = {
        0: list(range(4000, n, 4000)),                              # on slice edges
        1: [la(3), la(3) + 1, la(4) + 1, la(5) + 2, la(6), la(6) + 1],      # before / on / after; the sample alone
        2: list(range(15990, 16010)) + list(range(la(3) - 3, la(3) + 4)),   # one sample at a time across an edge and a look-ahead
        3: [la(3) + 2, la(7) - 1, la(7)],
        4: [n],                                                     # everything in one push
        5: [SLICE - 1, SLICE, SLICE + 1, 16000 - 1],
    }
    pos = {0: 100, 1: 100, 2: 0, 3: 0, 4: 0, 5: 0, 6: 100}
    pending = {s: [c for c in cuts[s] if c > pos[s]] + [n] for s in cuts}
    while any(pending.values()):
        entries = []
        for s in sorted(pending):
            if not pending[s]:
                continue
            c = pending[s].pop(0)
            if c <= pos[s]:
                continue
            entries.append((s, rec[s][pos[s]:c], False))
            pos[s] = c
        if entries:
            chk.push(entries)
    # every look-ahead has arrived except none past the end: the windows so far are all but the finish's
    for s in range(6):
        assert chk.received(s) == gm.scan_window_count(n), s
    # finishes: a zero-length push for streams 0..5 (nothing left to flush at this length), the short stream that never reached a window
    nw = chk.push([(s, rec[s][:0], True) for s in range(6)] + [(6, short[100:], True)])
    assert int(nw.sum()) == 0
    chk.close()
    gm.close()


def test_live_flush_at_finish(pkg, oracle):
    """the last slices' look-ahead samples never arrive: the push that finishes flushes them with the look-ahead read as 0"""
    gm = pkg.Model(os.path.join(MODELS, "l476_no_yes.kwsm"))
    lens = [24000, 24000 + G - 1, 28000 + 5, 16000]
    rec = [speech(oracle, 320 + i, n) for i, n in enumerate(lens)]
    ref = scan_windows(gm, rec)
    chk = LiveCheck(gm, len(rec))
    for i in range(len(rec)):
        chk.start(i, ref[i])
    nw = chk.push([(i, r, False) for i, r in enumerate(rec)])
    assert list(nw) == [2, 2, 3, 0]                                # slices whose look-ahead is missing wait
    nw = chk.push([(i, r[:0], True) for i, r in enumerate(rec)])
    assert list(nw) == [1, 1, 1, 1]
    chk.close()
    gm.close()


def test_live_state(pkg, oracle):
    """a second recording after finish and a stream after reset equal the scan of that recording alone; streams left out of pushes resume
    exactly; streams at very different positions share one push"""
    gm = pkg.Model(os.path.join(MODELS, "l476_no_yes.kwsm"))
    a, b, c = speech(oracle, 401, 52000 + 13), speech(oracle, 402, 37000), speech(oracle, 403, 800000)
    d = speech(oracle, 404, 30000)
    ref = scan_windows(gm, [a, b, c, d])
    chk = LiveCheck(gm, 4)
    # stream 0: a, finished, then b;  stream 1: part of c, reset, then b;  stream 2: c far ahead, stream 3 fresh, sharing pushes
    chk.start(0, ref[0])
    chk.start(1, ref[2])
    chk.start(2, ref[2])
    chk.push([(0, a[:30001], False), (1, c[:45000], False), (2, c[:700000], False)])
    chk.push([(0, a[30001:], True), (1, c[45000:45001], False)])
    chk.lv.reset([1])
    chk.start(0, ref[1])
    chk.start(1, ref[1])
    chk.start(3, ref[3])
    chk.push([(3, d[:5], False), (2, c[700000:700100], False), (0, b[:20000], False)])
    for k in range(5):                                              # stream 2 left out of five pushes, stream 1 joins late
        chk.push([(0, b[20000 + 3000 * k:23000 + 3000 * k], False), (3, d[5 + 5000 * k:5005 + 5000 * k], False)])
    chk.push([(1, b, True), (2, c[700100:], True), (3, d[25005:], True), (0, b[35000:], True)])
    for s, want in ((0, ref[1]), (1, ref[1]), (2, ref[2]), (3, ref[3])):
        got = chk.result(s)
        assert got[0].shape[0] == want[0].shape[0] and (bits(got[0]) == bits(want[0])).all(), s
    # reset of every stream part-way through a recording: a new recording on each starts from fresh state
    for s in range(4):
        chk.start(s, ref[2])
    chk.push([(s, c[:50000 + 4001 * s], False) for s in range(4)])
    chk.lv.reset()
    for s in range(4):
        chk.start(s, ref[3])
    chk.push([(s, d[:10000 + 7 * s], False) for s in range(4)])
    chk.push([(s, d[10000 + 7 * s:], True) for s in range(4)])
    chk.close()
    gm.close()


def test_live_scale_many_streams(pkg, oracle):
    """512 streams x 60 s in 100 ms packets (600 pushes of 512 entries), every window bitwise against the scan.  Eight distinct contents,
    each on 64 streams; the audio is resident on the device and the pushes read it in place."""
    import torch
    gm = pkg.Model(os.path.join(MODELS, "l476_no_yes.kwsm"))
    n, S, pk = 60 * 16000, 512, 1600
    contents = [speech(oracle, 700 + i, n) for i in range(8)]
    contents[3][300000:] = 0
    ref = scan_windows(gm, contents)
    order = np.random.default_rng(4).permutation(np.arange(S) % 8)
    audio = torch.from_numpy(np.stack([contents[j] for j in order])).cuda()
    lv = gm.live_streams(S)
    L = gm.n_labels
    out = np.full((S, 237, L), SENTINEL, np.float32)
    got = np.zeros(S, np.int64)
    sc = torch.empty((S, L), dtype=torch.float32, device="cuda")
    streams = np.arange(S)
    for t in range(n // pk):
        offs = streams * n + t * pk
        fin = np.full(S, int(t == n // pk - 1))
        nw = lv.push_device(audio.data_ptr(), streams, offs, np.full(S, pk), sc.data_ptr(), finish=fin).astype(np.int64)
        assert nw.max() <= 1
        k = int(nw.sum())
        if k:
            idx = np.nonzero(nw)[0]
            out[idx, got[idx]] = sc[:k].cpu().numpy()
            got[idx] += 1
    torch.cuda.synchronize()
    assert (got == 237).all()
    for s, j in enumerate(order):
        assert (bits(out[s]) == bits(ref[j][0])).all(), (s, j)
    lv.close()
    gm.close()


@pytest.mark.parametrize("name", ["l476_no_yes_f32.kwsm", "cfg2_mfcc40_f32.kwsm", "l476_no_yes.kwsm"])
def test_live_fast_mode(name, pkg, oracle, recs):
    """KWS_MODE_FAST: every window bitwise the fast scan's (each tier works per window), float32 graphs within 1e-4 of the oracle, and the
    windows handed back summed over the pushes equal the scan's counts for the same recordings"""
    path = os.path.join(MODELS, name)
    gm, om = pkg.Model(path), OracleModel(oracle, path)
    gm.set_mode(pkg.MODE_FAST)
    sub = [recs[i] for i in (5, 9, 13, 14, 15, 28, 29, 30, 31)]
    ref = scan_windows(gm, sub)
    scan_fb, scan_ex = gm.fast_fallback_count(), gm.fast_exact_count()
    chk = LiveCheck(gm, len(sub), fast_counts=True)
    for i in range(len(sub)):
        chk.start(i, ref[i])
    run_random_chunking(chk, sub, np.random.default_rng(7))
    assert (chk.fallbacks, chk.exacts) == (scan_fb, scan_ex)
    assert scan_fb >= 1                                            # silence and DC take the guard's re-run path
    if gm.is_float:
        for i, rec in enumerate(sub):
            want = oracle_scan(om, rec)
            got = chk.result(i)[0]
            assert got.shape == want.shape
            assert np.abs(got - want).max(initial=0.0) <= FAST_SCORE_TOL, i
    chk.close()
    gm.close()


def test_live_refusals(pkg, oracle):
    import torch
    gm = pkg.Model(os.path.join(MODELS, "l476_no_yes.kwsm"))
    with pytest.raises(pkg.KwsError) as e:
        gm.live_streams(0)
    assert e.value.code == -20
    # a slicing is refused with the code the scan gives
    for sl in (4001, 100, 8000, 16000, 3200):
        try:
            gm.scan_window_count(40000, sl)
            code = 0
        except pkg.KwsError as x:
            code = x.code
        if code == 0:
            gm.live_streams(2, sl).close()
            continue
        with pytest.raises(pkg.KwsError) as e:
            gm.live_streams(2, sl)
        assert e.value.code == code, (sl, e.value.code, code)
    lv = gm.live_streams(4)
    rec = speech(oracle, 5, 40000)
    d = torch.from_numpy(rec).cuda()
    s = torch.full((16, gm.n_labels), SENTINEL, dtype=torch.float32, device="cuda")
    lv.push_device(d.data_ptr(), [0, 1], [0, 0], [9000, 17], s.data_ptr())
    before = [lv.window_count(i, 12345, True) for i in range(4)]
    bad = [
        dict(streams=[2, 2], offsets=[0, 0], lengths=[10, 10]),
        dict(streams=[1, 4], offsets=[0, 0], lengths=[10, 10]),
        dict(streams=[1, 99], offsets=[0, 0], lengths=[10, 10]),
    ]
    for kw in bad:
        with pytest.raises(pkg.KwsError) as e:
            lv.push_device(d.data_ptr(), kw["streams"], kw["offsets"], kw["lengths"], s.data_ptr())
        assert e.value.code == -20, kw
    with pytest.raises(pkg.KwsError) as e:
        lv.push_device(d.data_ptr(), [0], [0], [10], None)
    assert e.value.code == -20
    with pytest.raises(pkg.KwsError) as e:
        lv.push_device(None, [0], [0], [10], s.data_ptr())
    assert e.value.code == -20
    with pytest.raises(pkg.KwsError) as e:
        lv.window_count(4, 10)
    assert e.value.code == -20
    with pytest.raises(pkg.KwsError) as e:
        lv.reset([0, 4])
    assert e.value.code == -20
    assert [lv.window_count(i, 12345, True) for i in range(4)] == before        # refusals change no state
    torch.cuda.synchronize()
    assert (s.cpu().numpy() == SENTINEL).all()
    lv.close()
    gm.close()
