"""kws_scan_recordings_device: every window of whole recordings in continuous mode, one call, against the restated
run_classifier_continuous() (oracle/kws_oracle.c) fed slice by slice with the end-of-signal sample the contract in include/kws/kws.h
defines, and against the product's own stream API."""
import os
import sys

import numpy as np
import pytest

from kws_testlib import MODELS, ROOT, OracleModel, bits
from scan_testlib import SLICE, moving_average, oracle_scan, pack, recordings, speech, wrap_sample

pytestmark = pytest.mark.gpu

FAST_SCORE_TOL = 1e-4
F32_SCORE_TOL = 1e-6
# the MFE-block graph of tests/test_gpu_mfe_model.py (tools/make_golden.py: MFE_MODEL_KW): no shipped model uses that block
MFE_KW = dict(seed=77, blocks=((8, 3, 7), (4, 3, 7)), n_labels=3, dsp_block="mfe")
EXACT_MODELS = ["l476_no_yes.kwsm", "l476_no_yes_f32.kwsm", "l432_trick_or_treat.kwsm", "cfg2_mfcc40_int8.kwsm", "cfg5_dscnn_mfcc40_f32.kwsm", "mfe"]


@pytest.fixture(scope="module")
def pkg():
    sys.path.insert(0, ROOT)
    import torch  # noqa: F401
    from __graft_entry__ import load_package
    return load_package()


@pytest.fixture(scope="module")
def recs(oracle):
    return recordings(oracle)


def model_path(name, tmp_path):
    if name != "mfe":
        return os.path.join(MODELS, name)
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from synth_model import synth_model_blob
    p = str(tmp_path / "mfe.kwsm")
    open(p, "wb").write(synth_model_blob(**MFE_KW))
    return p


def scan(pkg, gm, pcm, offs, lens, want_raw=True):
    import torch
    W = [gm.scan_window_count(int(n)) for n in lens]
    n = sum(W)
    d = torch.from_numpy(pcm).cuda()
    s = torch.full((max(n, 1), gm.n_labels), -7.0, dtype=torch.float32, device="cuda")
    r = torch.full((max(n, 1), gm.n_labels), -7.0, dtype=torch.float32, device="cuda") if want_raw else None
    gm.scan_recordings_device(d.data_ptr(), offs, lens, s.data_ptr(), r.data_ptr() if want_raw else None)
    torch.cuda.synchronize()
    s = s.cpu().numpy()[:n]
    r = r.cpu().numpy()[:n] if want_raw else None
    starts = np.concatenate([[0], np.cumsum(W)]).astype(np.int64)
    return W, starts, s, r


def check_exact(om, recs, W, starts, s, r, is_float=False):
    """int8 graphs: bit for bit; float32 graphs: within 1e-6 (the exact mode's float softmax uses the device expf, kws.h).  Raw scores
    through the reference's moving average give the scores, bit for bit, and the oracle's."""
    for i, rec in enumerate(recs):
        want = oracle_scan(om, rec)
        assert want.shape[0] == W[i], (i, want.shape, W[i])
        got = s[starts[i]:starts[i + 1]]
        same = (lambda a, b: np.abs(a - b).max(initial=0.0) <= F32_SCORE_TOL) if is_float else (lambda a, b: (bits(a) == bits(b)).all())
        assert same(got, want), i
        if r is not None:
            ma = moving_average(r[starts[i]:starts[i + 1]])
            assert (bits(ma) == bits(got)).all() and same(ma, want), i


@pytest.mark.parametrize("name", EXACT_MODELS)
def test_scan_exact_matches_the_continuous_oracle(name, pkg, oracle, recs, tmp_path):
    path = model_path(name, tmp_path)
    gm, om = pkg.Model(path), OracleModel(oracle, path)
    pcm, offs, lens = pack(recs, seed=3)
    W, starts, s, r = scan(pkg, gm, pcm, offs, lens)
    assert W[:7] == [0, 0, 0, 0, 0, 1, 1] and W[13] == 237
    check_exact(om, recs, W, starts, s, r, gm.is_float)
    gm.close()


@pytest.mark.parametrize("name", ["l476_no_yes.kwsm", "cfg2_mfcc40_f32.kwsm", "mfe"])
def test_scan_matches_the_stream_api(name, pkg, oracle, recs, tmp_path):
    """The same recordings through kws_streams_step_device, one fresh stream batch (S = 1) per recording, end_of_signal as defined."""
    import torch
    path = model_path(name, tmp_path)
    gm = pkg.Model(path)
    grow = int(np.float32(0.02) * np.float32(16000))
    sub = [recs[i] for i in (4, 5, 6, 7, 8, 9, 10, 12, 14, 15, 28, 29, 30, 31)]
    pcm, offs, lens = pack(sub, seed=5)
    W, starts, s, _ = scan(pkg, gm, pcm, offs, lens, want_raw=False)
    out = torch.empty((1, gm.n_labels), dtype=torch.float32, device="cuda")
    eos = torch.empty(1, dtype=torch.float32, device="cuda")
    for i, rec in enumerate(sub):
        sb = pkg.StreamBatch(gm, 1)
        got = []
        for k in range(rec.size // SLICE):
            sl = torch.from_numpy(np.ascontiguousarray(rec[k * SLICE:(k + 1) * SLICE])).cuda()
            eos.fill_(float(wrap_sample(rec, k, SLICE, grow)))
            if sb.step_device(sl.data_ptr(), SLICE, out.data_ptr(), eos.data_ptr()):
                torch.cuda.synchronize()
                got.append(out.cpu().numpy()[0].copy())
        sb.close()
        got = np.array(got, np.float32).reshape(-1, gm.n_labels)
        assert got.shape[0] == W[i]
        assert (bits(got) == bits(s[starts[i]:starts[i + 1]])).all(), i
    gm.close()


def test_scan_twenty_minute_recording(pkg, oracle):
    """4 797 windows of one recording: the moving average's running sum drifts over the run exactly as the reference's does"""
    path = os.path.join(MODELS, "l476_no_yes.kwsm")
    gm, om = pkg.Model(path), OracleModel(oracle, path)
    rec = speech(oracle, 901, 20 * 60 * 16000)
    rec[5_000_000:5_400_000] = 0
    pcm, offs, lens = pack([rec], seed=9)
    W, starts, s, r = scan(pkg, gm, pcm, offs, lens)
    assert W == [4797]
    check_exact(om, [rec], W, starts, s, r)
    gm.close()


@pytest.mark.parametrize("name", ["l476_no_yes_f32.kwsm", "cfg2_mfcc40_f32.kwsm", "l476_no_yes.kwsm", "cfg2_mfcc40_int8.kwsm"])
def test_scan_fast_mode(name, pkg, oracle, recs):
    """KWS_MODE_FAST: float32 graphs within 1e-4 of the oracle on every window; int8 graphs held to the rule the stream API's fast-mode
    test applies.  Silence and DC recordings take the guard's re-run path."""
    path = os.path.join(MODELS, name)
    gm, om = pkg.Model(path), OracleModel(oracle, path)
    gm.set_mode(pkg.MODE_FAST)
    sub = recs[:16] + recs[28:35]
    pcm, offs, lens = pack(sub, seed=11)
    W, starts, s, _ = scan(pkg, gm, pcm, offs, lens, want_raw=False)
    n_prod = n_diff = 0
    for i, rec in enumerate(sub):
        want = oracle_scan(om, rec)
        got = s[starts[i]:starts[i + 1]]
        assert got.shape == want.shape
        if not got.size:
            continue
        err = np.abs(got - want).max(axis=1)
        n_prod += err.size
        if gm.is_float:
            assert err.max() <= FAST_SCORE_TOL, (i, float(err.max()))
        else:
            n_diff += int((err > 0).sum())
            assert err.max() <= 2.5 / 256, (i, float(err.max()))
        if not rec.any():                                              # digital silence: constant columns -> the exact re-run
            assert err.max() <= (1e-6 if gm.is_float else 0.0), i
    assert n_prod > 300
    if not gm.is_float:
        assert n_diff <= max(2, n_prod // 50), (n_diff, n_prod)
    assert gm.fast_fallback_count() >= 1
    gm.close()


def test_scan_scale_many_recordings(pkg, oracle):
    """512 recordings x 60 s (121 344 windows: several chunks of the window stage) in exact mode, every window against the oracle.
    Eight distinct contents, each placed 64 times at different offsets and positions in the call."""
    path = os.path.join(MODELS, "l476_no_yes.kwsm")
    gm, om = pkg.Model(path), OracleModel(oracle, path)
    n = 60 * 16000
    contents = [speech(oracle, 700 + i, n) for i in range(8)]
    contents[3][300000:] = 0
    want = [oracle_scan(om, c) for c in contents]
    order = np.random.default_rng(4).permutation(np.arange(512) % 8)
    pcm, offs, lens = pack([contents[j] for j in order], seed=13, max_gap=9)
    W, starts, s, r = scan(pkg, gm, pcm, offs, lens)
    assert sum(W) == 512 * 237
    for i, j in enumerate(order):
        assert (bits(s[starts[i]:starts[i + 1]]) == bits(want[j])).all(), (i, j)
        assert (bits(moving_average(r[starts[i]:starts[i + 1]])) == bits(want[j])).all(), (i, j)
    gm.close()


def test_scan_refusals_and_empty_calls(pkg, oracle):
    import torch
    gm = pkg.Model(os.path.join(MODELS, "l476_no_yes.kwsm"))
    rec = speech(oracle, 5, 40000)
    d = torch.from_numpy(rec).cuda()
    s = torch.full((16, gm.n_labels), -7.0, dtype=torch.float32, device="cuda")
    # a slicing the stream API refuses is refused with the same code
    for sl in (4001, 100, 8000, 16000):
        sb = pkg.StreamBatch(gm, 1)
        code = 0
        x = torch.zeros(sl, dtype=torch.int16, device="cuda")
        try:
            for _ in range(6):
                sb.step_device(x.data_ptr(), sl, s.data_ptr())
        except pkg.KwsError as e:
            code = e.code
        sb.close()
        if code == 0:
            gm.scan_recordings_device(d.data_ptr(), [0], [rec.size], s.data_ptr(), slice_samples=sl)
            continue
        with pytest.raises(pkg.KwsError) as e:
            gm.scan_recordings_device(d.data_ptr(), [0], [rec.size], s.data_ptr(), slice_samples=sl)
        assert e.value.code == code, (sl, e.value.code, code)
        with pytest.raises(pkg.KwsError) as e:
            gm.scan_window_count(rec.size, sl)
        assert e.value.code == code
    torch.cuda.synchronize()
    with pytest.raises(pkg.KwsError) as e:
        gm.scan_recordings_device(d.data_ptr(), [0], [rec.size], None)
    assert e.value.code == -20
    s.fill_(-7.0)
    gm.scan_recordings_device(d.data_ptr(), [], [], s.data_ptr())
    gm.scan_recordings_device(d.data_ptr(), [0, 5, 7], [15999, 100, 0], s.data_ptr(), s.data_ptr())
    torch.cuda.synchronize()
    assert (s.cpu().numpy() == -7.0).all()
    gm.close()
