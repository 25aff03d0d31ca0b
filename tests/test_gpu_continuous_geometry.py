"""-m gpu: continuous mode at every slicing and frame geometry of the grid (tests/continuous_geometry.py) -- the stream API, the recording
scan and live sessions against the oracle's kwso_continuous_step fed slice by slice (continuous_geometry.oracle_scan), and each other.
Comparison rules: int8 graphs bit for bit, float32 graphs within 1e-6 in exact mode; raw scores through the reference moving average give
the scores bit for bit; KWS_MODE_FAST: float32 within 1e-4, int8 under test_gpu_scan.py::test_scan_fast_mode's flip rule."""
import sys

import numpy as np
import pytest

import continuous_geometry as cg
from kws_testlib import ROOT, OracleModel, bits
from live_testlib import LiveCheck, run_random_chunking, scan_windows
from scan_testlib import moving_average, pack

pytestmark = pytest.mark.gpu

F32_SCORE_TOL = 1e-6
FAST_SCORE_TOL = 1e-4
CASES = [(name, sl) for name in cg.GRID for sl in cg.GRID[name][1]]
FAST_CASES = [(name, sl) for name in ("l476", "l476_f32") for sl in (2000, 4160, 8000)]


@pytest.fixture(scope="module")
def pkg():
    sys.path.insert(0, ROOT)
    import torch  # noqa: F401
    from __graft_entry__ import load_package
    return load_package()


@pytest.fixture(scope="module")
def model_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("geometry_models")


def _setup(pkg, oracle, model_dir, name, sl):
    path = cg.model_path(name, model_dir)
    om = OracleModel(oracle, path)
    lay = cg.slice_walk(*cg.geometry(om.cfg, om.n_features), sl)
    assert isinstance(lay, cg.Layout), (name, sl)
    return pkg.Model(path), om, lay


def _same(gm):
    if gm.is_float:
        return lambda a, b: a.shape == b.shape and np.abs(a - b).max(initial=0.0) <= F32_SCORE_TOL
    return lambda a, b: a.shape == b.shape and (bits(a) == bits(b)).all()


def _scan(gm, recs, sl, want_raw=True, seed=3):
    import torch
    pcm, offs, lens = pack(recs, seed=seed)
    W = [gm.scan_window_count(int(n), sl) for n in lens]
    n = sum(W)
    d = torch.from_numpy(pcm).cuda()
    s = torch.full((max(n, 1), gm.n_labels), -7.0, dtype=torch.float32, device="cuda")
    r = torch.full((max(n, 1), gm.n_labels), -7.0, dtype=torch.float32, device="cuda")
    gm.scan_recordings_device(d.data_ptr(), offs, lens, s.data_ptr(), r.data_ptr() if want_raw else None, slice_samples=sl)
    torch.cuda.synchronize()
    s, r = s.cpu().numpy(), r.cpu().numpy()
    starts = np.concatenate([[0], np.cumsum(W)]).astype(np.int64)
    return W, [(s[starts[i]:starts[i + 1]], r[starts[i]:starts[i + 1]]) for i in range(len(recs))]


def _oracle(om, rec, sl):
    w, k, rc = cg.oracle_scan(om, rec, sl)
    assert k is None, (k, rc)
    return w


@pytest.mark.parametrize("name,sl", CASES)
def test_counts_and_scan_against_the_oracle(name, sl, pkg, oracle, model_dir):
    """window counts of the scan, of a live session and of the oracle equal the restatement's; every window of recordings at the layout's
    edges (packed at odd offsets between noise) against the oracle, raw scores through the moving average bit for bit"""
    gm, om, lay = _setup(pkg, oracle, model_dir, name, sl)
    long_s = 61 if sl == cg.GRID[name][1][0] else 0                # one long recording per model
    recs = cg.test_audio(oracle, lay, seed=5, long_s=long_s)
    lv = gm.live_streams(1, sl)
    try:
        for r in recs:
            assert gm.scan_window_count(r.size, sl) == lv.window_count(0, r.size, True) == lay.windows(r.size), (r.size, lay)
    finally:
        lv.close()
    W, got = _scan(gm, recs, sl)
    same = _same(gm)
    for i, rec in enumerate(recs):
        want = _oracle(om, rec, sl)
        assert want.shape[0] == W[i] == lay.windows(rec.size), (i, rec.size, want.shape, W[i])
        s, r = got[i]
        assert same(s, want), (i, rec.size, lay)
        assert (bits(moving_average(r)) == bits(s)).all(), (i, rec.size)
    gm.close()


@pytest.mark.parametrize("name,sl", CASES)
def test_streams_against_the_oracle(name, sl, pkg, oracle, model_dir):
    """a StreamBatch of 3 streams of different audio in lock step, each step's end_of_signal the look-ahead sample of each stream's
    recording (0 past its end), for enough steps that the ring's head wraps at least twice; every produced step against the oracle"""
    import torch
    gm, om, lay = _setup(pkg, oracle, model_dir, name, sl)
    steps = lay.k_full + 2 * (-(-lay.ring_rows // lay.nf1)) + 3
    n = steps * sl
    recs = [cg.speech(oracle, 40 + j, n + lay.grow + 5) for j in range(3)]
    recs[1] = recs[1][:n + lay.grow - 1]                          # its last look-ahead sample lies just past its end
    recs[2][n // 3:] = 0                                          # goes silent
    want = [_oracle(om, r, sl) for r in recs]
    sb = pkg.StreamBatch(gm, 3)
    try:
        out = torch.zeros((3, gm.n_labels), dtype=torch.float32, device="cuda")
        w = 0
        for k in range(steps):
            sl_host = np.stack([r[k * sl:(k + 1) * sl] for r in recs])
            p = [k * sl + sl + (lay.grow if k > 0 else 0) - 1 for _ in recs]
            eos = np.float32([np.float32(r[q]) * np.float32(1.0 / 32768.0) if q < r.size else 0.0 for r, q in zip(recs, p)])
            d = torch.from_numpy(np.ascontiguousarray(sl_host)).cuda()
            e = torch.from_numpy(eos).cuda()
            produced = sb.step_device(d.data_ptr(), sl, out.data_ptr(), e.data_ptr())
            torch.cuda.synchronize()
            assert produced == (k >= lay.k_full), (k, lay)
            if produced:
                got = out.cpu().numpy()
                for j in range(3):
                    assert _same(gm)(got[j:j + 1], want[j][w:w + 1]), (k, j, lay)
                w += 1
        assert w == want[0].shape[0] == lay.windows(n)
    finally:
        sb.close()
    gm.close()


@pytest.mark.parametrize("name,sl", CASES)
def test_live_against_the_scan(name, sl, pkg, oracle, model_dir):
    """random chunkings into a live session, every push checked against the scan bit for bit (live_testlib.LiveCheck), every stream
    finished; then 1-sample packets across a slice edge and across a look-ahead sample"""
    gm, om, lay = _setup(pkg, oracle, model_dir, name, sl)
    recs = cg.test_audio(oracle, lay, seed=9)
    ref = scan_windows(gm, recs, sl)
    chk = LiveCheck(gm, len(recs), sl)
    try:
        for i in range(len(recs)):
            chk.start(i, ref[i])
        run_random_chunking(chk, recs, np.random.default_rng(17))
        for i, r in enumerate(recs):
            s, _ = chk.result(i)
            assert s.shape[0] == lay.windows(r.size), (i, r.size)
        # one stream, single samples at the edges: slice k_full + 1's last sample, then the look-ahead sample of slice k_full + 1
        rec = cg.speech(oracle, 77, (lay.k_full + 4) * sl + lay.grow)
        chk.start(0, scan_windows(gm, [rec], sl)[0])
        edge = (lay.k_full + 2) * sl
        ahead = edge + lay.grow - 1
        cuts = sorted({edge - 1, edge, edge + 1, ahead - 1, ahead, ahead + 1})
        pos = 0
        for c in cuts:
            if c > pos:
                chk.push([(0, rec[pos:c], False)])
                pos = c
            chk.push([(0, rec[pos:pos + 1], False)])
            pos += 1
        chk.push([(0, rec[pos:], True)])
        assert chk.result(0)[0].shape[0] == lay.windows(rec.size)
        assert _same(gm)(chk.result(0)[0], _oracle(om, rec, sl))
    finally:
        chk.close()
    gm.close()


def test_refusals_agree_across_the_apis(pkg, oracle, model_dir):
    """every refused slicing of the grid: kws_scan_window_count, the scan, kws_live_create and the stream API's step all refuse it with
    the listed code"""
    import torch
    for name, (src, acc, refused) in cg.GRID.items():
        gm = pkg.Model(cg.model_path(name, model_dir))
        for sl, (code, rule) in refused.items():
            d = torch.zeros(5 * sl + 8, dtype=torch.int16, device="cuda")
            s = torch.zeros((64, gm.n_labels), dtype=torch.float32, device="cuda")
            codes = []
            for call in (lambda: gm.scan_window_count(40 * sl, sl),
                         lambda: gm.scan_recordings_device(d.data_ptr(), [1], [4 * sl], s.data_ptr(), None, slice_samples=sl),
                         lambda: gm.live_streams(2, sl).close()):
                with pytest.raises(pkg.KwsError) as ei:
                    call()
                codes.append(ei.value.code)
            sb = pkg.StreamBatch(gm, 1)
            try:
                with pytest.raises(pkg.KwsError) as ei:
                    for _ in range(8):
                        sb.step_device(d.data_ptr(), sl, s.data_ptr())
                codes.append(ei.value.code)
            finally:
                sb.close()
            torch.cuda.synchronize()
            assert codes == [code] * 4, (name, sl, rule, codes)
        gm.close()


def test_fast_mode_refused_on_general_geometries(pkg, model_dir):
    """set_mode(FAST) is refused wherever the plan is general (the fast kernel serves tuned plans only): those grid models run exact only"""
    for name in ("stride10", "stride10_f32", "odd_stride_fft512", "fft128_win51", "two_s_40f"):
        gm = pkg.Model(cg.model_path(name, model_dir))
        with pytest.raises(pkg.KwsError):
            gm.set_mode(pkg.MODE_FAST)
        gm.close()


@pytest.mark.parametrize("name,sl", FAST_CASES)
def test_fast_mode_at_other_slicings(name, sl, pkg, oracle, model_dir):
    """KWS_MODE_FAST for the shipped models at slicings other than 4000: the scan against the oracle under the fast rules, a live session
    bitwise equal to the fast scan with the same fallback count, and the stream API against the oracle"""
    import torch
    gm, om, lay = _setup(pkg, oracle, model_dir, name, sl)
    gm.set_mode(pkg.MODE_FAST)
    recs = cg.test_audio(oracle, lay, seed=13)
    W, got = _scan(gm, recs, sl, want_raw=False)
    scan_fb = gm.fast_fallback_count()
    n_prod = n_diff = 0
    for i, rec in enumerate(recs):
        want = _oracle(om, rec, sl)
        s = got[i][0]
        assert s.shape == want.shape, i
        if not s.size:
            continue
        err = np.abs(s - want).max(axis=1)
        n_prod += err.size
        if gm.is_float:
            assert err.max() <= FAST_SCORE_TOL, (i, float(err.max()))
        else:
            n_diff += int((err > 0).sum())
            assert err.max() <= 2.5 / 256, (i, float(err.max()))
    if not gm.is_float:
        assert n_diff <= max(2, n_prod // 50), (n_diff, n_prod)
    # live: the same recordings, bitwise the fast scan, the same fallback count
    ref = scan_windows(gm, recs, sl)
    chk = LiveCheck(gm, len(recs), sl, fast_counts=True)
    try:
        for i in range(len(recs)):
            chk.start(i, ref[i])
        run_random_chunking(chk, recs, np.random.default_rng(23))
        assert chk.fallbacks == scan_fb, (chk.fallbacks, scan_fb)
    finally:
        chk.close()
    # streams: one stream through the longest recording
    rec = max(recs, key=lambda r: r.size)
    want = _oracle(om, rec, sl)
    sb = pkg.StreamBatch(gm, 1)
    try:
        out = torch.zeros((1, gm.n_labels), dtype=torch.float32, device="cuda")
        rows = []
        for k in range(rec.size // sl):
            q = k * sl + sl + (lay.grow if k > 0 else 0) - 1
            e = torch.tensor([np.float32(rec[q]) * np.float32(1.0 / 32768.0) if q < rec.size else 0.0], dtype=torch.float32, device="cuda")
            d = torch.from_numpy(np.ascontiguousarray(rec[k * sl:(k + 1) * sl])).cuda()
            if sb.step_device(d.data_ptr(), sl, out.data_ptr(), e.data_ptr()):
                torch.cuda.synchronize()
                rows.append(out.cpu().numpy()[0].copy())
        rows = np.array(rows, np.float32).reshape(-1, gm.n_labels)
        assert rows.shape == want.shape
        err = np.abs(rows - want).max(axis=1, initial=0.0)
        assert err.max(initial=0.0) <= (FAST_SCORE_TOL if gm.is_float else 2.5 / 256)
        assert gm.is_float or int((err > 0).sum()) <= max(2, err.size // 50)
    finally:
        sb.close()
    gm.close()
