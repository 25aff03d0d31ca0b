"""-m gpu: MFE-block models at the general DSP shapes of tests/mfe_general_shapes.py through every entry point, against the oracle
(kwso_extract_mfe and the model-level functions, pinned to the compiled reference by tests/test_mfe_general_pin.py) and the fixture of the
reference's own numbers (tests/golden/mfe_general_l432.npz).  Bars: features and int8 tensors bit for bit with identical NaN patterns, no clip
skipped or masked; int8 scores and float32 logits bit for bit; float32 scores within 1e-6.  Every test fails where kws_create refuses the blob."""
import os
import subprocess
import sys

import numpy as np
import pytest

import mfe_general_shapes as G
from kws_testlib import GOLDEN, ROOT, OracleContinuous, OracleModel, bits

pytestmark = pytest.mark.gpu
UNSUPPORTED_MODEL, DSP_ERROR = -18, -5
N_DISTINCT = 40
SLICE_A = 3999            # shape A's frames overlap: a slice of 4000 samples would end inside a frame (tests/continuous_geometry.py, "past")


def same(a, b):
    """same bits, or NaN on both sides"""
    a = np.asarray(a, np.float32); b = np.asarray(b, np.float32)
    return bool(((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())


def close(a, b, tol=1e-6):
    return bool(((np.abs(a - b) <= tol) | (np.isnan(a) & np.isnan(b))).all())


@pytest.fixture(scope="module")
def pkg():
    sys.path.insert(0, ROOT)
    import torch  # noqa: F401
    from __graft_entry__ import load_package
    return load_package()


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, G.FIXTURE))


@pytest.fixture(scope="module")
def refs(oracle, tmp_path_factory):
    """(path, oracle model, 40 distinct clips -- the fixture's four first --, scores, features, int8 tensors) per (shape, float32?), computed once"""
    out, made = str(tmp_path_factory.mktemp("mfe_general")), {}

    def get(tag, f32=False):
        if (tag, f32) not in made:
            path = G.write_model(tag, out, f32)
            om = OracleModel(oracle, path)
            clips = np.concatenate([G.fixture_clips(oracle, tag), oracle.synth(23, 0, N_DISTINCT - G.FIXTURE_CLIPS, clip_len=om.raw_sample_count)])
            s, f, q = om.run_batch(clips, want_features=True)
            for a in (clips, s, f, q):
                a.setflags(write=False)
            made[(tag, f32)] = (path, om, clips, s, f, q)
        return made[(tag, f32)]
    return get


def dev_run(gm, clips, want_q=True):
    import torch
    B = len(clips)
    d = torch.from_numpy(np.array(clips)).to("cuda:0")
    s = torch.zeros((B, gm.n_labels), dtype=torch.float32, device="cuda:0")
    f = torch.zeros((B, gm.n_features), dtype=torch.float32, device="cuda:0")
    q = torch.zeros((B, gm.n_features), dtype=torch.int8, device="cuda:0") if (want_q and not gm.is_float) else None
    gm.run_classifier_batch_device(d.data_ptr(), B, s.data_ptr(), f.data_ptr(), q.data_ptr() if q is not None else None)
    torch.cuda.synchronize()
    return s.cpu().numpy(), f.cpu().numpy(), (q.cpu().numpy() if q is not None else None)


CASES = [("A", False), ("A", True), ("B", False), ("B", True), ("C", False), ("D", False), ("E1", False), ("E2", False), ("F", False)]


@pytest.mark.parametrize("tag,f32", CASES, ids=["%s_%s" % (t, "f32" if f else "i8") for t, f in CASES])
def test_batch_calls_follow_the_oracle_and_the_fixture(tag, f32, pkg, refs, golden):
    import torch
    path, om, clips, s_ref, f_ref, q_ref = refs(tag, f32)
    gm = pkg.Model(path)
    assert gm.mfcc_kernel == G.SPECTRAL[tag] and gm.n_features == G.ROWS_COLS[tag][0] * G.ROWS_COLS[tag][1]
    assert np.isnan(f_ref[2]).all() and (tag == "E2" or np.isfinite(f_ref[:2]).all())           # NaN clips are in, and not alone
    for B in ((1, 3, 8) if tag == "F" else (1, 3, 1000)):                                         # 1 000: a persistent grid strides over the clips
        idx = (np.arange(B) * 7 + (B == 1)) % N_DISTINCT
        s, f, q = dev_run(gm, clips[idx])
        assert same(f, f_ref[idx]), (tag, B)
        if f32:
            assert close(s, s_ref[idx]), (tag, B, np.nanmax(np.abs(s - s_ref[idx])))
        else:
            assert (q == q_ref[idx]).all() and (bits(s) == bits(s_ref[idx])).all(), (tag, B)
    n = G.FIXTURE_CLIPS                                                                           # the reference's own numbers
    s, f, q = dev_run(gm, clips[:n])
    assert same(f, golden[tag + "_features"])
    if not f32:
        assert (q == golden[tag + "_q"]).all() and (bits(s) == bits(golden[tag + "_scores"])).all()
    # the stage calls, on every distinct clip
    d = torch.from_numpy(np.array(clips)).to("cuda:0")
    B, F, L = len(clips), gm.n_features, gm.n_labels
    new = lambda *shape, dt=torch.float32: torch.zeros(shape, dtype=dt, device="cuda:0")
    mel, en, ft, ft2, ft3, sc, sc2 = new(B, F), new(B, G.ROWS_COLS[tag][0]), new(B, F), new(B, F), new(B, F), new(B, L), new(B, L)
    qt = None if f32 else new(B, F, dt=torch.int8)
    gm.mfe_batch_device(d.data_ptr(), B, mel.data_ptr(), en.data_ptr())
    gm.extract_mfe_batch_device(d.data_ptr(), B, ft.data_ptr())
    gm.extract_mfcc_batch_device(d.data_ptr(), B, ft2.data_ptr(), None if f32 else qt.data_ptr())
    gm.cmvn_inference_batch_device(mel.data_ptr(), B, sc.data_ptr(), ft3.data_ptr())
    gm.run_inference_batch_device(ft.data_ptr(), B, sc2.data_ptr())
    torch.cuda.synchronize()
    c0 = om.cfg.copy(pre_cof=0.0)
    want = [om.o.mfe(x, c0) for x in clips[:8]]
    assert (bits(mel.cpu().numpy()[:8]) == bits(np.stack([m.reshape(-1) for m, _ in want]))).all()
    assert (bits(en.cpu().numpy()[:8]) == bits(np.stack([e for _, e in want]))).all()
    for t in (ft, ft2, ft3):
        assert same(t.cpu().numpy(), f_ref), tag
    for t in (sc, sc2):
        assert close(t.cpu().numpy(), s_ref) if f32 else (bits(t.cpu().numpy()) == bits(s_ref)).all(), tag
    if f32:
        lg = new(B, L)
        gm.nn_f32_batch_device(ft.data_ptr(), B, sc.data_ptr(), lg.data_ptr())
        torch.cuda.synchronize()
        z = np.stack([[t for t in om.nn_invoke_f32(x, taps=True)[1] if len(t) == L][-2] for x in f_ref])      # the tensor SOFTMAX reads
        assert same(lg.cpu().numpy(), z)
    else:
        assert (qt.cpu().numpy() == q_ref).all()
        s, f, q = gm.run_classifier_batch(clips[:8], want_features=True)                           # host buffers
        assert same(f, f_ref[:8]) and (q == q_ref[:8]).all() and (bits(s) == bits(s_ref[:8])).all()
    gm.close()


def test_tuned_chunks_equal_the_cooperative_kernel_on_shape_a(dev_pkg, refs, monkeypatch):
    import torch
    path, om, clips, s_ref, f_ref, q_ref = refs("A")
    d = torch.from_numpy(np.array(clips)).to("cuda:0")

    def stage(gm):
        B = len(clips)
        mel = torch.zeros((B, gm.n_features), dtype=torch.float32, device="cuda:0")
        gm.mfe_batch_device(d.data_ptr(), B, mel.data_ptr())
        torch.cuda.synchronize()
        return (mel.cpu().numpy(),) + dev_run(gm, clips)
    gm = dev_pkg.Model(path)
    assert gm.mfcc_kernel == "kws_mfcc8_kernel (chunked)"
    a = stage(gm)
    gm.close()
    monkeypatch.setenv("KWS_DEV_GENERIC_NO_TUNED_SPECTRAL", "1")
    gm = dev_pkg.Model(path)
    assert gm.mfcc_kernel == "kws_spectral_lds_kernel"
    b = stage(gm)
    gm.close()
    assert (bits(a[0]) == bits(b[0])).all() and same(a[2], b[2]) and (a[3] == b[3]).all() and (bits(a[1]) == bits(b[1])).all()
    assert same(a[2], f_ref) and (a[3] == q_ref).all()


def test_lds_form_equals_the_global_memory_form(dev_pkg, refs, monkeypatch):
    """the two forms of the normalisation on the shapes both can run (development switch KWS_DEV_MFE_NORM_GLOBAL)"""
    for tag in ("A", "D", "E2"):
        path, om, clips, s_ref, f_ref, q_ref = refs(tag)
        monkeypatch.setenv("KWS_DEV_MFE_NORM_GLOBAL", "1")
        gm = dev_pkg.Model(path)
        s, f, q = dev_run(gm, clips)
        gm.close()
        monkeypatch.delenv("KWS_DEV_MFE_NORM_GLOBAL")
        assert same(f, f_ref) and (q == q_ref).all() and (bits(s) == bits(s_ref)).all(), tag


def _stream_loop(pkg, gm, rec, slice_samples):
    """kws_streams_step_device over one recording, slice by slice: the scores of the steps that produced a window"""
    import torch
    sb = pkg.StreamBatch(gm, 1)
    sc = torch.empty((1, gm.n_labels), dtype=torch.float32, device="cuda")
    out = []
    for k in range(rec.size // slice_samples):
        d = torch.from_numpy(np.ascontiguousarray(rec[None, k * slice_samples:(k + 1) * slice_samples])).cuda()
        if sb.step_device(d.data_ptr(), slice_samples, sc.data_ptr()):
            torch.cuda.synchronize()
            out.append(sc.cpu().numpy()[0].copy())
    sb.close()
    return np.array(out, np.float32).reshape(-1, gm.n_labels)


def test_continuous_mode_streams_scan_and_live_on_shape_a(pkg, oracle, refs):
    import torch
    from live_testlib import LiveCheck, run_random_chunking, scan_windows
    import continuous_geometry as cg
    from scan_testlib import speech
    path, om = refs("A")[:2]
    gm = pkg.Model(path)
    S, n_steps = 3, 12
    audio = oracle.synth(15, 0, S * 3).reshape(S, 3 * 16000)
    sb = pkg.StreamBatch(gm, S)
    # the oracle's walk with each slice's frames free to read on into the recording (kwso_continuous_step_ex: a 320-sample frame reads 64 samples
    # the 256-point transform drops, and the last frame of a 3 999-sample slice ends one sample past it)
    want = [cg.oracle_scan(om, audio[s, :n_steps * SLICE_A], SLICE_A) for s in range(S)]
    assert all(w[1] is None for w in want)
    scores = torch.empty((S, gm.n_labels), dtype=torch.float32, device="cuda")
    n_produced = 0
    for k in range(n_steps):
        sl = np.ascontiguousarray(audio[:, k * SLICE_A:(k + 1) * SLICE_A])
        d = torch.from_numpy(sl).cuda()
        produced = sb.step_device(d.data_ptr(), SLICE_A, scores.data_ptr())
        torch.cuda.synchronize()
        if produced:
            got = scores.cpu().numpy()
            for s in range(S):
                assert (bits(got[s]) == bits(want[s][0][n_produced])).all(), (k, s)
            n_produced += 1
    assert n_produced == want[0][0].shape[0] == n_steps - 3
    sb.close()
    # recordings of 2 - 4 s: the scan == the stream loop == the oracle's walk; live pushes in ragged packets == the scan
    recs = [speech(oracle, 31, 32000 + 17), speech(oracle, 32, 48000), speech(oracle, 33, 63999)]
    ref = scan_windows(gm, recs, SLICE_A)
    for r, (sc, _) in zip(recs, ref):
        loop = _stream_loop(pkg, gm, r, SLICE_A)
        assert sc.shape[0] == loop.shape[0] > 0 and (bits(sc) == bits(loop)).all()
        assert (bits(sc) == bits(cg.oracle_scan(om, r, SLICE_A)[0])).all()
    chk = LiveCheck(gm, len(recs), SLICE_A)
    for i in range(len(recs)):
        chk.start(i, ref[i])
    run_random_chunking(chk, recs, np.random.default_rng(5))
    for i in range(len(recs)):
        assert (bits(chk.result(i)[0]) == bits(ref[i][0])).all()
    chk.close()
    gm.close()


def test_continuous_mode_on_shape_b_is_refused_as_the_oracle_refuses_it(pkg, oracle, refs):
    """Shape B's frames are two strides long (512 samples every 256): whatever the slice length, the last frame a grown slice claims ends past the
    slice, the reference's get_data of it fails, and the oracle refuses the step; so does the library (EI_IMPULSE_DSP_ERROR), as it does for an
    MFCC block of that geometry.  One-shot windows of the shape are served (the batch test above)."""
    import torch
    path, om = refs("B")[:2]
    gm = pkg.Model(path)
    audio = oracle.synth(15, 0, 1).reshape(-1)
    oc = OracleContinuous(om)
    oc.init()
    rcs = [oc.step(audio[k * 4000:(k + 1) * 4000])[0] for k in range(2)]
    assert rcs[0] == 0 and rcs[1] != 0
    sb = pkg.StreamBatch(gm, 1)
    sc = torch.empty((1, gm.n_labels), dtype=torch.float32, device="cuda")
    with pytest.raises(pkg.KwsError) as e:
        for k in range(2):
            d = torch.from_numpy(np.ascontiguousarray(audio[None, k * 4000:(k + 1) * 4000])).cuda()
            sb.step_device(d.data_ptr(), 4000, sc.data_ptr())
    torch.cuda.synchronize()
    assert e.value.code == DSP_ERROR
    sb.close()
    gm.close()


def test_one_shot_windows_slide_and_slide_live_on_shape_a(pkg, oracle, refs):
    import torch
    import slide_live_testlib as SL
    from slide_testlib import batch_device, cut_windows, pack, recordings, slide, speech
    path, om = refs("A")[:2]
    gm = pkg.Model(path)
    clip, stride = gm.clip_samples, gm.frame_stride_samples
    assert (clip, stride) == (16000, 160)
    for hop in (stride, 5 * stride, 4000):
        recs = recordings(oracle, clip, hop, seed=4)
        pcm, offs, lens = pack(recs, seed=hop)
        d = torch.from_numpy(pcm).cuda()
        sd, fd, n = slide(gm, d, offs, lens, hop, SL.DIRECT)
        ss, fs, n2 = slide(gm, d, offs, lens, hop, SL.SHARED)
        win, W = cut_windows(recs, clip, hop)
        sb, fb = batch_device(gm, win)
        assert n == n2 == sum(W) == win.shape[0] > 0
        assert same(fd, fs) and same(fd, fb.cpu().numpy()) and (bits(sd) == bits(ss)).all() and (bits(sd) == bits(sb.cpu().numpy())).all(), hop
    hop = 5 * stride
    recs = [speech(oracle, 41, clip + 3 * hop + 7), speech(oracle, 42, clip - 1), speech(oracle, 43, 20000)]
    for flags in (SL.DIRECT, SL.SHARED):
        ref = SL.Reference(gm, recs, hop, flags)
        sess = gm.slide_streams(len(recs), hop, flags)
        fd = SL.Feeder(gm, sess, ref)
        while any(fd.left(s) for s in range(len(recs))):                       # 20 ms packets
            fd.push([(s, min(320, fd.left(s))) for s in range(len(recs)) if fd.left(s)])
        assert fd.finished()
        sess.close()
    gm.close()


def test_bank_of_an_int8_model_and_its_float32_twin_on_shape_a(pkg, refs):
    import torch
    (p8, _, clips, s8, f8, _), (pf, _, _, sf, ff, _) = refs("A"), refs("A", True)
    m8, mf = pkg.Model(p8), pkg.Model(pf)
    bank = pkg.Bank([m8, mf])
    B = len(clips)
    d = torch.from_numpy(np.array(clips)).to("cuda:0")
    s = [torch.zeros((B, m.n_labels), dtype=torch.float32, device="cuda:0") for m in (m8, mf)]
    f = torch.zeros((B, m8.n_features), dtype=torch.float32, device="cuda:0")
    bank.run_classifier_batch_device(d.data_ptr(), B, [t.data_ptr() for t in s], f.data_ptr())
    torch.cuda.synchronize()
    own8, ownf = dev_run(m8, clips), dev_run(mf, clips)
    assert same(f.cpu().numpy(), own8[1]) and same(own8[1], ownf[1]) and same(own8[1], f8)
    assert (bits(s[0].cpu().numpy()) == bits(own8[0])).all() and same(s[1].cpu().numpy(), ownf[0])
    assert (bits(own8[0]) == bits(s8)).all() and close(ownf[0], sf)
    bank.close(); m8.close(); mf.close()


def test_ragged_clips_of_1_to_98_frames_on_shape_a(pkg, oracle, refs):
    import torch
    path, om, clips = refs("A")[:3]
    gm = pkg.Model(path)
    frames = [1, 17, 49, 50, 98, 17, 98, 1]
    lens = np.array([320 + 160 * n for n in frames], np.uint64)
    assert [gm.window_frame_count(int(n)) for n in lens] == frames
    src = [clips[4 + i][:int(n)] for i, n in enumerate(lens)]
    offs = np.concatenate([[3], 3 + np.cumsum(lens[:-1] + 5)]).astype(np.uint64)                # odd offsets: the clips are staged
    buf = np.full(int(offs[-1] + lens[-1]) + 8, 30000, np.int16)
    for o, c in zip(offs, src):
        buf[int(o):int(o) + c.size] = c
    B, F = len(src), gm.n_features
    t = {k: torch.full((B, w), 0xFF, dtype=torch.uint8, device="cuda:0") for k, w in (("s", 4 * gm.n_labels), ("f", 4 * F), ("q", F))}
    gm.run_classifier_ragged_device(torch.from_numpy(buf).cuda().data_ptr(), offs, lens, t["s"].data_ptr(), t["f"].data_ptr(), t["q"].data_ptr())
    torch.cuda.synchronize()
    s, f, q = t["s"].cpu().numpy().view(np.float32), t["f"].cpu().numpy().view(np.float32), t["q"].cpu().numpy().view(np.int8)
    for i, c in enumerate(src):
        feat = np.zeros(F, np.float32)
        part = oracle.extract_mfe(c, om.cfg)
        feat[:part.size] = part
        qi = om.quantize_input(feat)
        assert same(f[i], feat) and (q[i] == qi).all() and (bits(s[i]) == bits(om.dequantize(om.nn_invoke(qi)))).all(), (i, frames[i])
    gm.close()


def test_sdk_entry_points_in_a_fresh_process():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "mfe_general_sdk_worker.py")], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                         text=True, timeout=600)
    assert out.returncode == 0 and "OK" in out.stdout, out.stdout[-2000:] + out.stderr[-3000:]


def test_refusals_and_the_tuned_model(pkg, refs):
    for tag in ("A", "F"):
        gm = pkg.Model(refs(tag)[0])
        with pytest.raises(pkg.KwsError) as e:
            gm.set_mode(pkg.MODE_FAST)
        assert e.value.code == UNSUPPORTED_MODEL and len(str(e.value)) > 20
        gm.close()
    with pytest.raises(pkg.KwsError) as e:
        pkg.Model(blob=G.blob(G.RADIX7_KW))
    assert e.value.code == UNSUPPORTED_MODEL and "radix" in str(e.value)
    with pytest.raises(pkg.KwsError) as e:
        pkg.Model(blob=G.blob(G.FEW_FILTERS_KW))
    assert e.value.code == UNSUPPORTED_MODEL and "32 filters" in str(e.value)
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from make_golden import MFE_MODEL_KW
    gm = pkg.Model(blob=G.blob(MFE_MODEL_KW))
    assert gm.mfcc_kernel == "kws_mfcc8_kernel"
    gm.set_mode(pkg.MODE_FAST)
    gm.close()
