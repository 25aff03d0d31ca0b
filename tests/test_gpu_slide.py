"""kws_slide_recordings_device: run_classifier() at every position of whole recordings, one window every hop samples, in one call --
against the oracle on the windows cut out on the CPU, against the product's own kws_run_classifier_batch_device on the same windows,
and each path (direct: every window's rows computed for it; shared: rows computed once per recording and position) against the other."""
import os
import sys

import numpy as np
import pytest

from kws_testlib import MODELS, ROOT, OracleModel, bits, synth_model_blob
from slide_testlib import MFE_KW, SENTINEL, batch_device, cut_windows, n_speech_like, pack, recordings, slide, speech

pytestmark = pytest.mark.gpu

FAST_SCORE_TOL = 1e-4          # BASELINE.json's grant for KWS_MODE_FAST
F32_SCORE_TOL = 1e-6           # the project's bar for exact-mode float32 scores (the float softmax uses the device expf, kws.h)
AUTO, DIRECT, SHARED = 0, 1, 2
CLIP = 16000
EXACT_MODELS = ["l476_no_yes.kwsm", "l432_trick_or_treat.kwsm", "l476_no_yes_f32.kwsm", "cfg2_mfcc40_int8.kwsm", "cfg5_dscnn_mfcc40_f32.kwsm", "mfe",
                "stride10ms_win31", "odd_stride_fft512"]
# two general-shape DSP configurations of tests/test_gpu_generic_dsp.py (its BLOCKS and CASES): overlapping frames (98 of them; the tuned
# spectral kernel in chunks + the general cmvnw), and 321-sample frames every 161 at fft 512 (the general kernels' sample-by-sample loads)
GENERAL = {
    "stride10ms_win31": dict(frame_stride=0.01, win_size=31),
    "odd_stride_fft512": dict(fft_length=512, frame_length=0.0200625, frame_stride=0.0100625, win_size=31),
}
GENERAL_BLOCKS = dict(blocks=((8, 3, 7), (4, 3, 7)), n_labels=3)
FAST_MODELS = ["l476_no_yes.kwsm", "cfg2_mfcc40_f32.kwsm", "mfe"]
# in units the test resolves per model: "s" = the frame stride, "c" = the clip
HOPS = ["s", "2s", 4000, 1000, 7, 1, "c", "c+13"]


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
                kw = MFE_KW if name == "mfe" else dict(GENERAL_BLOCKS, seed=3, **GENERAL[name])
                path = str(tmp_path_factory.mktemp("slide") / (name + ".kwsm"))
                open(path, "wb").write(synth_model_blob(**kw))
            made[name] = (pkg.Model(path), OracleModel(oracle, path))
        return made[name]

    yield get
    for gm, _ in made.values():
        gm.close()


def resolve_hop(hop, gm):
    return {"s": gm.frame_stride_samples, "2s": 2 * gm.frame_stride_samples, "c": gm.clip_samples, "c+13": gm.clip_samples + 13}.get(hop, hop)


def check_plan(gm, lens, hop, name):
    """what the plan says AUTO runs, and that it is the cheaper path in rows"""
    p = gm.slide_plan(lens, hop)
    assert p["n_windows"] == sum(gm.slide_window_count(int(n), hop) for n in lens)
    assert p["rows_direct"] == p["n_windows"] * gm.n_frames
    assert p["rows_first"] == (0 if name == "mfe" else p["n_windows"])
    assert p["phases"] == gm.frame_stride_samples // np.gcd(hop, gm.frame_stride_samples)
    assert p["path"] == (SHARED if p["rows_shared"] + p["rows_first"] < p["rows_direct"] else DIRECT)
    for flags in (DIRECT, SHARED):
        assert gm.slide_plan(lens, hop, flags)["path"] == flags
    return p


@pytest.mark.parametrize("hop", HOPS, ids=[str(h) for h in HOPS])
@pytest.mark.parametrize("name", EXACT_MODELS)
def test_slide_exact_matches_the_oracle_on_every_path(name, hop, pkg, oracle, models):
    import torch
    gm, om = models(name)
    assert gm.clip_samples == CLIP
    hop = resolve_hop(hop, gm)
    recs = recordings(oracle, CLIP, hop)
    pcm, offs, lens = pack(recs, seed=3)
    windows, W = cut_windows(recs, CLIP, hop)
    # lengths 0, clip - 1, clip, clip + 1, clip + hop - 1, clip + hop, clip + 3 hop + 7 (at hop 1, clip + 1 is clip + hop)
    assert W[:7] == [0, 0, 1, 2 if hop == 1 else 1, 1, 2, (3 * hop + 7) // hop + 1]
    p = check_plan(gm, lens, hop, name)
    if hop in (gm.frame_stride_samples, 2 * gm.frame_stride_samples):
        assert p["path"] == SHARED and p["phases"] == 1
    if hop >= CLIP:
        assert p["path"] == DIRECT
    s_ref, f_ref, _ = om.run_batch(windows, want_features=True)
    d = torch.from_numpy(pcm).cuda()
    out = {flags: slide(gm, d, offs, lens, hop, flags) for flags in (AUTO, DIRECT, SHARED)}
    s_b, f_b = batch_device(gm, windows)
    for flags, (s, f, n) in out.items():
        assert n == sum(W) == windows.shape[0]
        assert (bits(f) == bits(f_ref)).all(), (name, hop, flags, int((bits(f) != bits(f_ref)).any(axis=1).sum()))
        if gm.is_float:
            assert np.abs(s - s_ref).max() <= F32_SCORE_TOL, (name, hop, flags, float(np.abs(s - s_ref).max()))
        else:
            assert (bits(s) == bits(s_ref)).all(), (name, hop, flags)
        # the paths among themselves, and the product's own batch call on the windows: bit for bit, float32 scores included
        assert (bits(s) == bits(out[AUTO][0])).all() and (bits(f) == bits(out[AUTO][1])).all(), (name, hop, flags)
        assert (bits(s) == bits(s_b.cpu().numpy())).all() and (bits(f) == bits(f_b.cpu().numpy())).all(), (name, hop, flags)
    # without the feature matrix: the same scores
    s, _, _ = slide(gm, d, offs, lens, hop, SHARED, want_features=False)
    assert (bits(s) == bits(out[SHARED][0])).all(), (name, hop)


@pytest.mark.parametrize("name", ["l476_no_yes.kwsm", "mfe"])
def test_slide_plan_reports_the_path_that_runs(name, pkg, models):
    gm, _ = models(name)
    stride, clip, nf = gm.frame_stride_samples, gm.clip_samples, gm.n_frames
    lens = [clip - 1, clip, clip + 10 * stride, 60 * 16000]
    p = gm.slide_plan(lens, stride)
    n = 1 + 11 + (60 * 16000 - clip) // stride + 1
    assert p["path"] == SHARED and p["n_windows"] == n and p["phases"] == 1
    pre = 0 if name == "mfe" else 1
    assert p["rows_first"] == pre * n and p["rows_shared"] == n - 3 + 3 * (nf - pre) and p["rows_direct"] == n * nf
    assert p["rows_shared"] + p["rows_first"] < p["rows_direct"] // 20
    for hop in (clip, clip + 13, 2 * clip):
        assert gm.slide_plan(lens, hop)["path"] == DIRECT
    for hop in (stride, 5 * stride, 4000, 1000, 7, 1):
        q = gm.slide_plan(lens, hop)
        assert q["path"] == SHARED and q["rows_shared"] + q["rows_first"] < q["rows_direct"], hop


def test_slide_across_the_window_chunk(pkg, oracle, models):
    """33 001 windows of one recording at hop 1: two chunks of the window stage, 320 phases.  Against the batch call on the windows gathered
    on the device, bit for bit, and the windows around the chunk boundary against the oracle."""
    import torch
    gm, om = models("l476_no_yes.kwsm")
    rec = speech(oracle, 77, CLIP + 33000)
    pcm, offs, lens = pack([rec], seed=5)
    assert gm.slide_plan(lens, 1)["path"] == SHARED
    d = torch.from_numpy(pcm).cuda()
    s, f, n = slide(gm, d, offs, lens, 1, AUTO)
    assert n == 33001
    s2, f2, _ = slide(gm, d, offs, lens, 1, DIRECT)
    assert (bits(s) == bits(s2)).all() and (bits(f) == bits(f2)).all()
    windows = d[int(offs[0]):int(offs[0]) + rec.size].unfold(0, CLIP, 1)
    assert windows.shape == (33001, CLIP)
    s_b, f_b = batch_device(gm, windows, piece=4096)
    assert torch.equal(torch.from_numpy(s).cuda().view(torch.int32), s_b.view(torch.int32))
    assert torch.equal(torch.from_numpy(f).cuda().view(torch.int32), f_b.view(torch.int32))
    lo, hi = 32760, 32776
    s_ref, f_ref, _ = om.run_batch(np.stack([rec[w:w + CLIP] for w in range(lo, hi)]), want_features=True)
    assert (bits(f[lo:hi]) == bits(f_ref)).all() and (bits(s[lo:hi]) == bits(s_ref)).all()


@pytest.mark.parametrize("name", FAST_MODELS)
def test_slide_fast_mode(name, pkg, oracle, models):
    """KWS_MODE_FAST: scores within 1e-4 of the oracle on the speech-like recordings, the two paths bit-identical, and the guard's count
    the same on a second identical call.  The silent recordings take the guard's re-run."""
    import torch
    gm, om = models(name)
    hop = gm.frame_stride_samples
    recs = recordings(oracle, CLIP, hop)
    pcm, offs, lens = pack(recs, seed=11)
    windows, W = cut_windows(recs, CLIP, hop)
    n_speech = sum(W[:n_speech_like(recs)])
    s_ref = om.run_batch(windows)
    d = torch.from_numpy(pcm).cuda()
    gm.set_mode(pkg.MODE_FAST)
    try:
        s1, f1, n = slide(gm, d, offs, lens, hop, SHARED)
        c1 = gm.fast_fallback_count()
        s2, f2, _ = slide(gm, d, offs, lens, hop, SHARED)
        c2 = gm.fast_fallback_count()
        s3, f3, _ = slide(gm, d, offs, lens, hop, DIRECT)
        c3 = gm.fast_fallback_count()
    finally:
        gm.set_mode(pkg.MODE_EXACT)
    assert n == sum(W) and n_speech > 100
    err = np.abs(s1 - s_ref).max(axis=1)
    print("%s: fast mode, %d windows, max |score - oracle| speech-like %.3g, all %.3g, fallbacks %d" % (name, n, err[:n_speech].max(), err.max(), c1))
    assert err[:n_speech].max() <= FAST_SCORE_TOL, (name, float(err[:n_speech].max()))
    assert (bits(s1) == bits(s2)).all() and (bits(f1) == bits(f2)).all() and c1 == c2
    assert (bits(s1) == bits(s3)).all() and (bits(f1) == bits(f3)).all() and c1 == c3
    if name != "mfe":                                   # (the MFE block's fast form is its exact one: no guard, no count)
        assert c1 >= 1


def test_slide_refusals_and_empty_calls(pkg, oracle, models):
    import torch
    gm, _ = models("l476_no_yes.kwsm")
    rec = speech(oracle, 5, 40000)
    d = torch.from_numpy(rec).cuda()
    s = torch.full((128, gm.n_labels), SENTINEL, dtype=torch.float32, device="cuda")
    f = torch.full((128, gm.n_features), SENTINEL, dtype=torch.float32, device="cuda")
    for kw in (dict(hop_samples=0), dict(hop_samples=320, flags=3), dict(hop_samples=320, flags=-1)):
        with pytest.raises(pkg.KwsError) as e:
            gm.slide_recordings_device(d.data_ptr(), [0], [rec.size], scores_ptr=s.data_ptr(), **kw)
        assert e.value.code == -20, kw
    with pytest.raises(pkg.KwsError) as e:
        gm.slide_recordings_device(d.data_ptr(), [0], [rec.size], 320, None, f.data_ptr())
    assert e.value.code == -20
    with pytest.raises(pkg.KwsError) as e:
        gm.slide_window_count(rec.size, 0)
    assert e.value.code == -20
    with pytest.raises(pkg.KwsError) as e:
        gm.slide_plan([rec.size], 320, flags=9)
    assert e.value.code == -20
    for flags in (AUTO, DIRECT, SHARED):
        gm.slide_recordings_device(d.data_ptr(), [], [], 320, s.data_ptr(), f.data_ptr(), flags=flags)
        gm.slide_recordings_device(d.data_ptr(), [0, 5, 7], [15999, 100, 0], 320, s.data_ptr(), f.data_ptr(), flags=flags)
    torch.cuda.synchronize()
    assert (s.cpu().numpy() == SENTINEL).all() and (f.cpu().numpy() == SENTINEL).all()
