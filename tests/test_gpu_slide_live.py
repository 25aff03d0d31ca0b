"""kws_slide_live_*: live streams of one-shot windows.  Every push is checked on the spot (slide_live_testlib.Feeder): its counts against
window_count, its rows bitwise against the next rows of kws_slide_recordings_device on the stream's whole recording, the rows behind its
last one untouched -- on the retained-row path, on the direct path, in exact and in fast mode -- and, so that the suite does not rest on
the product's slide alone, against the oracle on the windows cut out on the CPU."""
import ctypes
import os
import sys

import numpy as np
import pytest

from kws_testlib import MODELS, ROOT, OracleModel, bits, synth_model_blob
from slide_live_testlib import AUTO, DIRECT, SHARED, Feeder, Reference, auto_path, edge_lengths, paths_for, served, speech, windows_of
from slide_testlib import MFE_KW, SENTINEL, cut_windows, slide

pytestmark = pytest.mark.gpu

FAST_SCORE_TOL = 1e-4          # BASELINE.json's grant for KWS_MODE_FAST
F32_SCORE_TOL = 1e-6           # the project's bar for exact-mode float32 scores (tests/test_gpu_slide.py)
CLIP = 16000
# the general-shape DSP configuration of tests/test_gpu_slide.py: 321-sample frames every 161 at fft 512
ODD_STRIDE = dict(blocks=((8, 3, 7), (4, 3, 7)), n_labels=3, seed=3, fft_length=512, frame_length=0.0200625, frame_stride=0.0100625, win_size=31)
CHUNK_MODELS = ["l476_no_yes.kwsm", "cfg2_mfcc40_f32.kwsm", "mfe", "odd_stride_fft512"]
# in units the test resolves per model: "s" = the frame stride, "c" = the clip
CHUNK_HOPS = ["s", "2s", 4000, "48s", "49s", 1000, "c+13"]
FAST_MODELS = ["l476_no_yes.kwsm", "cfg2_mfcc40_f32.kwsm", "mfe"]


@pytest.fixture(scope="module")
def pkg():
    sys.path.insert(0, ROOT)
    import torch  # noqa: F401
    from __graft_entry__ import load_package
    return load_package()


@pytest.fixture(scope="module")
def models(pkg, oracle, tmp_path_factory):
    """name -> (product model, oracle model), created once per module"""
    made = {}

    def get(name):
        if name not in made:
            if name.endswith(".kwsm"):
                path = os.path.join(MODELS, name)
            else:
                path = str(tmp_path_factory.mktemp("slide_live") / (name + ".kwsm"))
                open(path, "wb").write(synth_model_blob(**(MFE_KW if name == "mfe" else ODD_STRIDE)))
            made[name] = (pkg.Model(path), OracleModel(oracle, path))
        return made[name]

    yield get
    for gm, _ in made.values():
        gm.close()


def resolve_hop(hop, gm):
    s, c = gm.frame_stride_samples, gm.clip_samples
    return {"s": s, "2s": 2 * s, "48s": 48 * s, "49s": 49 * s, "c": c, "c+13": c + 13}.get(hop, hop)


def pre_of(name):
    return 0 if name == "mfe" else 1          # an MFE block has no pre-emphasis: frame 0 is shared too


class Session:
    """a slide-live session that is closed whatever the test does"""

    def __init__(self, gm, S, hop, flags=AUTO):
        self.gm, self.args = gm, (S, hop, flags)

    def __enter__(self):
        self.sess = self.gm.slide_streams(*self.args)
        return self.sess

    def __exit__(self, *exc):
        self.sess.close()


@pytest.mark.parametrize("hop", CHUNK_HOPS, ids=[str(h) for h in CHUNK_HOPS])
@pytest.mark.parametrize("name", CHUNK_MODELS)
def test_random_chunkings_return_the_slides_rows_on_every_path(name, hop, pkg, oracle, models):
    """8 streams of lengths around every edge of the window count, random packets of 1 sample to 1.5 clips to random subsets: every push
    returns the slide's next rows, on AUTO and on each forced path that is served (so the paths are bitwise equal to each other)"""
    gm, _ = models(name)
    assert gm.clip_samples == CLIP
    hop = resolve_hop(hop, gm)
    pre = pre_of(name)
    recs = [speech(oracle, 300 + i, n) for i, n in enumerate(edge_lengths(CLIP, hop))]
    ref = Reference(gm, recs, hop)
    assert ref.W[:6] == [0, 0, 1, 1, 1, 2]
    if not served(gm, hop, pre):
        with pytest.raises(pkg.KwsError) as e:
            gm.slide_streams(8, hop, SHARED)
        assert e.value.code == -20
    for k, flags in enumerate(paths_for(gm, hop, pre)):
        with Session(gm, 8, hop, flags) as sess:
            assert sess.path == (auto_path(gm, hop, pre) if flags == AUTO else flags), (name, hop, flags, sess.path)
            fd = Feeder(gm, sess, ref, want_features=True)
            fd.feed_randomly(np.random.default_rng(1000 * k + hop), CLIP * 3 // 2)
            assert fd.pushes >= 3
    stride = gm.frame_stride_samples
    if hop in (stride, 2 * stride):
        assert auto_path(gm, hop, pre) == SHARED
    if hop > CLIP or hop % stride:
        assert auto_path(gm, hop, pre) == DIRECT


@pytest.mark.parametrize("flags", [AUTO, DIRECT], ids=["auto", "direct"])
@pytest.mark.parametrize("hop", ["s", 4000], ids=["s", "4000"])
def test_packet_boundaries(hop, flags, pkg, oracle, models):
    """packets that end one sample before, on and after a window's last sample; one sample at a time across two such samples; zero-length
    entries; a push that completes no window on fresh streams; and everything in one push"""
    gm, _ = models("l476_no_yes.kwsm")
    hop = resolve_hop(hop, gm)
    n = CLIP + 3 * hop + 5
    recs = [speech(oracle, 400 + i, n) for i in range(5)]
    ref = Reference(gm, recs, hop)
    last = [w * hop + CLIP - 1 for w in range(4)]                   # the last sample of windows 0 .. 3
    with Session(gm, 5, hop, flags) as sess:
        fd = Feeder(gm, sess, ref)
        assert fd.push([(s, 100) for s in range(5)]) == [0] * 5     # no window, fresh streams
        assert fd.push([(s, 0) for s in range(5)]) == [0] * 5       # zero-length entries only
        # streams 0 / 1 / 2: packets up to just before / on / just after the last sample of windows 0, 1 and 2; stream 4 joins with nothing
        for w in range(3):
            ends = [last[w], last[w] + 1, last[w] + 2]
            got = fd.push([(s, ends[s] - fd.pos[s]) for s in range(3)] + [(4, 0)])
            assert got == [0 if w == 0 else 1, 1, 1, 0], (w, got)
        # stream 3: up to two samples before window 0's last, then one sample at a time across it; the same across window 1's
        for w in range(2):
            fd.push([(3, last[w] - 1 - fd.pos[3])])
            got = [fd.push([(3, 1), (4, 0)])[0] for _ in range(4)]
            assert got == [0, 1, 0, 0], (w, got)
        fd.push([(s, fd.left(s)) for s in range(5)])
        assert fd.finished()
    with Session(gm, 5, hop, flags) as sess:                        # everything in one push
        fd = Feeder(gm, sess, ref)
        assert fd.push([(s, n) for s in (3, 0, 4, 1, 2)]) == [4] * 5
        assert fd.finished()


def test_a_push_inside_the_dropped_gap(pkg, oracle, models):
    """hop = clip + 13: the 13 samples between two windows are dropped as they arrive -- in a push that lies wholly in the gap, in one that
    ends on the gap's last sample, and in one that spans it"""
    gm, _ = models("l476_no_yes.kwsm")
    hop = CLIP + 13
    recs = [speech(oracle, 500 + i, 2 * hop + CLIP + 4) for i in range(3)]
    ref = Reference(gm, recs, hop)
    assert ref.W == [3, 3, 3]
    with Session(gm, 3, hop) as sess:
        assert sess.path == DIRECT
        fd = Feeder(gm, sess, ref)
        assert fd.push([(0, CLIP), (1, CLIP + 5), (2, CLIP - 1)]) == [1, 1, 0]
        assert fd.push([(0, 5), (1, 8), (2, 3)]) == [0, 0, 1]       # stream 0: wholly in the gap; 1: up to the gap's end; 2: into the gap
        assert fd.push([(0, 8), (1, 1), (2, 11)]) == [0, 0, 0]
        assert fd.push([(0, CLIP - 1), (1, CLIP), (2, CLIP + 7)]) == [0, 1, 1]
        assert fd.push([(0, 1 + 13 + CLIP), (1, 6)]) == [2, 0]      # across a whole gap
        fd.push([(s, fd.left(s)) for s in range(3)])
        assert fd.finished()


@pytest.mark.parametrize("flags", [AUTO, DIRECT], ids=["auto", "direct"])
@pytest.mark.parametrize("name", ["l476_no_yes.kwsm", "cfg2_mfcc40_f32.kwsm"])
def test_rings_wrap(name, flags, pkg, oracle, models):
    """4 streams x 4 s at hop = stride in 10 ms packets: the carry ring wraps four times, the row ring about 150 times; and 2 streams where
    a 3 s packet follows ten 1-sample packets (a push much longer than either ring)"""
    gm, _ = models(name)
    hop = gm.frame_stride_samples
    recs = [speech(oracle, 600 + i, 4 * 16000) for i in range(4)] + [speech(oracle, 610 + i, 10 + 3 * 16000) for i in range(2)]
    ref = Reference(gm, recs, hop)
    with Session(gm, 6, hop, flags) as sess:
        assert sess.path == (SHARED if flags == AUTO else DIRECT)
        fd = Feeder(gm, sess, ref, want_features=True)
        for i in range(10):
            fd.push([(4, 1), (5, 1)])
        fd.push([(5, 3 * 16000), (4, 3 * 16000)])
        for p in range(400):
            fd.push([(s, 160) for s in range(4)])
        assert fd.finished() and fd.pushes == 411


def test_reset_left_out_streams_and_distant_positions(pkg, oracle, models):
    """a reset in mid-stream, then another recording; streams left out of several pushes resume exactly; streams at very different
    positions share a push"""
    gm, _ = models("l476_no_yes.kwsm")
    hop = gm.frame_stride_samples
    recs = [speech(oracle, 700 + i, n) for i, n in enumerate([40000, 30000, 25000, 36000, 28000])]
    ref = Reference(gm, recs, hop)
    with Session(gm, 4, hop) as sess:
        assert sess.path == SHARED
        fd = Feeder(gm, sess, ref, rec_of=[0, 1, 2, 3])
        fd.push([(0, 20000), (1, 17000), (2, 100), (3, 16500)])
        # stream 1 is reset in mid-stream and starts recording 4; host only, nothing else moves
        sess.reset([1])
        fd.restart(1, 4)
        assert sess.window_count(1, CLIP) == 1 and sess.window_count(0, hop) == 1
        # streams 2 and 3 are left out of several pushes
        for n in (333, 1, 5000, 320, 7):
            fd.push([(0, n), (1, n + 2000)])
        # very different positions in one push: stream 0 far along, stream 1 young, stream 2 before its first window, stream 3 resuming
        assert fd.pos[0] > 25000 and fd.pos[2] == 100
        fd.push([(2, 15899), (0, 4000), (3, 1), (1, 9000)])
        fd.push([(2, 1), (3, 19000)])
        fd.push([(s, fd.left(s)) for s in range(4)])
        assert fd.finished()
        sess.reset()                                                # all streams: every one starts over
        for s in range(4):
            fd.restart(s, (s + 1) % 4)
        fd.feed_randomly(np.random.default_rng(5), CLIP)


def test_two_sessions_and_slide_calls_interleave_on_one_handle(pkg, oracle, models):
    """two sessions on one handle at hops stride and 4000, and a kws_slide_recordings_device call at a third hop, interleaved push by push:
    each stays bitwise equal to its own reference (a session keeps nothing in the handle's slide scratch)"""
    gm, _ = models("l476_no_yes.kwsm")
    stride = gm.frame_stride_samples
    recs = [speech(oracle, 800 + i, n) for i, n in enumerate([33000, 24000, 40000])]
    ref_a, ref_b = Reference(gm, recs, stride), Reference(gm, recs, 4000)
    ref_c = Reference(gm, recs, 2 * stride, flags=SHARED)
    with Session(gm, 3, stride) as sa, Session(gm, 3, 4000) as sb:
        assert (sa.path, sb.path) == (SHARED, DIRECT)
        fa, fb = Feeder(gm, sa, ref_a), Feeder(gm, sb, ref_b)
        rng = np.random.default_rng(9)
        k = 0
        while not (fa.finished() and fb.finished()):
            for fd in (fa, fb):
                fd.push([(s, min(int(rng.integers(1, 6000)), fd.left(s))) for s in range(3)])
            s, f, _ = slide(gm, ref_c.d_pcm, ref_c.offs, ref_c.lens, 2 * stride, (SHARED, DIRECT)[k % 2])
            assert (bits(s) == bits(np.concatenate(ref_c.scores))).all() and (bits(f) == bits(np.concatenate(ref_c.features))).all()
            k += 1
        assert k >= 5


class OracleRows:
    """Reference's fields with the oracle's rows: run_batch on every window cut out on the CPU"""

    def __init__(self, om, recs, hop, ref):
        windows, W = cut_windows(recs, CLIP, hop)
        s, f, _ = om.run_batch(windows, want_features=True)
        cut = np.cumsum([0] + W)
        self.recs, self.hop, self.W = recs, hop, W
        self.offs, self.d_pcm = ref.offs, ref.d_pcm
        self.scores = [s[cut[i]:cut[i + 1]] for i in range(len(recs))]
        self.features = [f[cut[i]:cut[i + 1]] for i in range(len(recs))]


@pytest.mark.parametrize("name", ["l476_no_yes.kwsm", "mfe"])
def test_pushes_match_the_oracle_directly(name, pkg, oracle, models):
    """hop = 2 strides: the features of every returned window are bitwise OracleModel.run_batch on the window cut out on the CPU; scores by
    the rules of tests/test_gpu_slide.py (int8 bitwise, float32 within 1e-6)"""
    gm, om = models(name)
    hop = 2 * gm.frame_stride_samples
    recs = [speech(oracle, 900 + i, n) for i, n in enumerate([CLIP + 5 * hop + 3, 30000, CLIP, CLIP + hop])]
    ref = Reference(gm, recs, hop)
    rows = OracleRows(om, recs, hop, ref)
    assert sum(rows.W) > 30
    for flags in paths_for(gm, hop, pre_of(name)):
        with Session(gm, 4, hop, flags) as sess:
            fd = Feeder(gm, sess, rows, score_tol=F32_SCORE_TOL if gm.is_float else None)
            fd.feed_randomly(np.random.default_rng(31 + flags), 9000)


@pytest.mark.parametrize("name", FAST_MODELS)
def test_fast_mode_returns_the_fast_slides_rows_and_counts(name, pkg, oracle, models):
    """KWS_MODE_FAST: rows bitwise the fast slide's; fallback and exact counts summed over the pushes equal the slide's for the same
    recordings (a silent and a DC recording make sure at least one window is handed back); float graphs within 1e-4 of the oracle"""
    gm, om = models(name)
    hop = gm.frame_stride_samples
    recs = [speech(oracle, 950 + i, n) for i, n in enumerate([CLIP + 20 * hop + 1, 30000, CLIP - 1])]
    recs += [np.zeros(CLIP + 5 * hop, np.int16), np.full(CLIP + 3 * hop + 2, 1234, np.int16)]
    counted = name != "mfe"                             # (the MFE block's fast form is its exact one: no guard, no count)
    gm.set_mode(pkg.MODE_FAST)
    try:
        ref = Reference(gm, recs, hop)
        want = (gm.fast_fallback_count(), gm.fast_exact_count())
        for flags in (AUTO, DIRECT):
            with Session(gm, 5, hop, flags) as sess:
                fd = Feeder(gm, sess, ref)
                got = [0, 0]

                def tally(windows):
                    c = (gm.fast_fallback_count(), gm.fast_exact_count())
                    if counted and windows == 0:
                        assert c == (0, 0), c           # the counts describe the last push: none for a push without windows
                    got[0] += c[0]
                    got[1] += c[1]

                fd.feed_randomly(np.random.default_rng(77 + flags), 7000, after_push=tally)
                if counted:
                    assert tuple(got) == want, (name, flags, got, want)
    finally:
        gm.set_mode(pkg.MODE_EXACT)
    if counted:
        assert want[0] >= 1, want                       # at least one window was handed back
    if gm.is_float:
        windows, _ = cut_windows(recs, CLIP, hop)
        err = np.abs(np.concatenate(ref.scores) - om.run_batch(windows)).max()
        print("%s: fast mode, %d windows, max |score - oracle| %.3g, fallbacks %d, exact %d" % (name, windows.shape[0], err, want[0], want[1]))
        assert err <= FAST_SCORE_TOL, (name, float(err))


def test_refusals_change_nothing(pkg, oracle, models):
    import torch
    gm, _ = models("l476_no_yes.kwsm")
    stride = gm.frame_stride_samples
    for S, hop, flags in ((0, stride, AUTO), (1 << 30, stride, AUTO), (4, 0, AUTO), (4, (1 << 56) + 1, AUTO), (4, stride, 3), (4, stride, -1),
                          (4, 7, SHARED), (4, 1000, SHARED), (4, 49 * stride, SHARED), (4, CLIP, SHARED)):
        with pytest.raises(pkg.KwsError) as e:
            gm.slide_streams(S, hop, flags)
        assert e.value.code == -20, (S, hop, flags)
    rec = speech(oracle, 5, 40000)
    d = torch.from_numpy(rec).cuda()
    with Session(gm, 4, stride) as sess:
        s = torch.full((64, gm.n_labels), SENTINEL, dtype=torch.float32, device="cuda")
        f = torch.full((64, gm.n_features), SENTINEL, dtype=torch.float32, device="cuda")
        assert list(sess.push_device(d.data_ptr(), [0, 2], [0, 5], [15999, 9000], s.data_ptr(), f.data_ptr())) == [0, 0]
        before = [sess.window_count(k, 12345) for k in range(4)]
        L = sess.L
        sz = np.uint64
        st, off, ln, nw = (np.array(v, sz) for v in ([0, 2], [0, 0], [9000, 9000], [77, 77]))

        def p(a):
            return a.ctypes.data_as(ctypes.c_void_p)

        calls = {
            "duplicate": (2, p(np.array([1, 1], sz)), d.data_ptr(), p(off), p(ln), s.data_ptr(), f.data_ptr(), p(nw)),
            "range": (2, p(np.array([1, 4], sz)), d.data_ptr(), p(off), p(ln), s.data_ptr(), f.data_ptr(), p(nw)),
            "nullstreams": (2, None, d.data_ptr(), p(off), p(ln), s.data_ptr(), f.data_ptr(), p(nw)),
            "nulllengths": (2, p(st), d.data_ptr(), p(off), None, s.data_ptr(), f.data_ptr(), p(nw)),
            "nullcounts": (2, p(st), d.data_ptr(), p(off), p(ln), s.data_ptr(), f.data_ptr(), None),
            "nullscores": (2, p(st), d.data_ptr(), p(off), p(ln), None, f.data_ptr(), p(nw)),
            "nullpcm": (2, p(st), None, p(off), p(ln), s.data_ptr(), f.data_ptr(), p(nw)),
            "nulloffsets": (2, p(st), d.data_ptr(), None, p(ln), s.data_ptr(), f.data_ptr(), p(nw)),
            "toomany": (2, p(st), d.data_ptr(), p(off), p(np.array([9000, 1 << 60], sz)), s.data_ptr(), f.data_ptr(), p(nw)),
        }
        for case, args in calls.items():
            assert L.kws_slide_live_push_device(sess.sl, *args, None) == -20, case
        with pytest.raises(pkg.KwsError) as e:
            sess.reset([1, 4])
        assert e.value.code == -20
        for stream, n_new in ((4, 10), (0, 1 << 60)):
            with pytest.raises(pkg.KwsError) as e:
                sess.window_count(stream, n_new)
            assert e.value.code == -20
        torch.cuda.synchronize()
        assert [sess.window_count(k, 12345) for k in range(4)] == before
        assert list(nw) == [77, 77]
        assert (s.cpu().numpy() == SENTINEL).all() and (f.cpu().numpy() == SENTINEL).all()
        # the session still works: the streams go on from where they were
        assert list(sess.push_device(d.data_ptr(), [0, 2], [15999, 9005], [1 + stride, 7000 + stride], s.data_ptr(), f.data_ptr())) == [2, 2]
        torch.cuda.synchronize()
        assert windows_of(15999 + 1 + stride, CLIP, stride) == 2 and (s[:4].cpu().numpy() != SENTINEL).all() and (s[4:].cpu().numpy() == SENTINEL).all()
