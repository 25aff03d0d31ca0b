"""-m gpu: KWS_MODE_FAST (include/kws/kws.h) against the C oracle.  Bar (BASELINE.json north_star): float32 scores within 1e-4
of the reference's; int8 graphs exact from the int8 input tensor on, with the input-tensor flip rate reported and bounded.
Clips whose cmvnw is ill-conditioned must come out exactly as in KWS_MODE_EXACT (they are re-run by the exact kernels)."""
import multiprocessing as mp
import os

import numpy as np
import pytest

from kws_testlib import GOLDEN, MODELS, ROOT, Oracle, OracleModel, bits, special_clips

pytestmark = pytest.mark.gpu

FAST_SCORE_TOL = 1e-4          # north_star: "per-class scores match the reference C path within 1e-4 fp32"
EXACT_SCORE_TOL = 1e-6         # KWS_MODE_EXACT's float bar (device expf in the softmax)
FAST_FEATURE_TOL = 2e-3        # |feature - oracle| for clips the fast kernel keeps (well-conditioned cmvnw)
FAST_LOGIT_TOL = 4e-4          # |d(z_a - z_b)|: the 1e-4 score bar stated at the logits (|d score| <= 1/4 of it) -- it does not shrink when the softmax saturates


@pytest.fixture(scope="module")
def pkg():
    import sys
    sys.path.insert(0, ROOT)
    import torch  # noqa: F401
    from __graft_entry__ import load_package
    return load_package()


_W = {}


def _oracle_worker(args):
    path, seed, first, n = args
    if path not in _W:
        o = _W.setdefault("oracle", Oracle())
        _W[path] = OracleModel(o, path)
    om, o = _W[path], _W["oracle"]
    s, f, q = om.run_batch(o.synth(seed, first, n), want_features=True)
    z = np.zeros_like(s)
    if o.L.kwso_model_is_float(om.h):
        for i in range(n):
            _, taps = om.nn_invoke_f32(f[i], taps=True)
            z[i] = [t for t in taps if len(t) == om.n_labels][-2]            # the tensor SOFTMAX reads: the logits
    return first, s, f, q, z


def oracle_all(path, seed, B, chunk=512, want_logits=False):
    """scores, features, int8 tensors (and logits of float graphs) of synthetic clips [0, B) of `seed` from the oracle, one worker per host core"""
    om = OracleModel(Oracle(), path)
    s = np.zeros((B, om.n_labels), np.float32)
    f = np.zeros((B, om.n_features), np.float32)
    q = np.zeros((B, om.n_features), np.int8)
    z = np.zeros((B, om.n_labels), np.float32)
    jobs = [(path, seed, i, min(chunk, B - i)) for i in range(0, B, chunk)]
    with mp.get_context("spawn").Pool(len(os.sched_getaffinity(0))) as pool:
        for first, ss, ff, qq, zz in pool.imap_unordered(_oracle_worker, jobs):
            s[first:first + len(ss)], f[first:first + len(ss)], q[first:first + len(ss)], z[first:first + len(ss)] = ss, ff, qq, zz
    return (s, f, q, z) if want_logits else (s, f, q)


def pair_error(z, zo):
    """largest error of a logit DIFFERENCE per clip (what the softmax sees)"""
    dz = z.astype(np.float64) - zo.astype(np.float64)
    return np.abs(dz[:, :, None] - dz[:, None, :]).reshape(len(z), -1).max(axis=1)


def run_device(pkg, gm, mode, pcm_t, want_f=True):
    import torch
    n = pcm_t.shape[0]
    gm.set_mode(mode)
    s = torch.zeros((n, gm.n_labels), dtype=torch.float32, device="cuda:0")
    f = torch.zeros((n, gm.n_features), dtype=torch.float32, device="cuda:0") if want_f else None
    q = torch.zeros((n, gm.n_features), dtype=torch.int8, device="cuda:0") if (want_f and not gm.is_float) else None
    gm.run_classifier_batch_device(pcm_t.data_ptr(), n, s.data_ptr(), f.data_ptr() if want_f else None, q.data_ptr() if q is not None else None)
    torch.cuda.synchronize()
    return s.cpu().numpy(), (f.cpu().numpy() if want_f else None), (q.cpu().numpy() if q is not None else None)


@pytest.mark.parametrize("name", ["cfg2_mfcc40_f32.kwsm", "l476_no_yes_f32.kwsm"])
def test_fast_mode_float_scores_within_1e4_of_the_oracle_on_a_full_batch(name, pkg):
    """BASELINE configs[1] size: every one of 65 536 synthetic clips through the fused fast kernel and through the oracle."""
    import torch
    path = os.path.join(MODELS, name)
    gm = pkg.Model(path, device=0)
    assert gm.fast_is_fused
    B, seed = 65536, 4100
    pcm = torch.empty((B, 16000), dtype=torch.int16, device="cuda:0")
    pkg.synth_clips_device(seed, 0, B, 16000, pcm.data_ptr())
    z_t = torch.zeros((B, gm.n_labels), dtype=torch.float32, device="cuda:0")
    gm.set_logits_tap(z_t.data_ptr())
    s, f, _ = run_device(pkg, gm, pkg.MODE_FAST, pcm)
    n_fallback = gm.fast_fallback_count()
    z = z_t.cpu().numpy().copy()
    z_t.zero_()
    s2, _, _ = run_device(pkg, gm, pkg.MODE_FAST, pcm, want_f=False)           # scores only: the features never leave the chip
    z2 = z_t.cpu().numpy().copy()
    n_fb_scores_only = gm.fast_fallback_count()
    gm.set_logits_tap(None)
    so, fo, _, zo = oracle_all(path, seed, B, want_logits=True)
    d_s, d_f, d_z = np.abs(s - so).max(), np.abs(f - fo).max(), pair_error(z, zo).max()
    mx = so.max(axis=1)
    print("\n%s fast mode, %d clips: max |score - oracle| = %.3g, max |logit difference - oracle| = %.3g, max |feature - oracle| = %.3g, %d clips handed back "
          "(%d when only the scores are asked for); the oracle's winning score: median %.2f, > 0.999 on %.1f %% of the clips"
          % (name, B, d_s, d_z, d_f, n_fallback, n_fb_scores_only, np.median(mx), 100.0 * (mx > 0.999).mean()))
    assert not np.isnan(s).any()
    assert d_s <= FAST_SCORE_TOL
    assert d_z <= FAST_LOGIT_TOL                          # every clip, at the logits: no saturation to hide behind
    assert (mx > 0.999).mean() < 0.05                     # ... and the model's softmax is not saturated anyway
    assert d_f <= FAST_FEATURE_TOL
    # without the feature matrix the one launch knows the clip's own scores: it may keep a (saturated) clip that the feature-emitting launch,
    # which assumes the largest p (1 - p) there is, hands on -- never the other way round
    n_fallback2 = n_fb_scores_only
    assert n_fallback2 <= n_fallback and np.abs(s2 - s).max() <= FAST_SCORE_TOL and pair_error(z2, zo).max() <= FAST_LOGIT_TOL
    assert n_fallback < B // 100                         # synthetic clips are well-conditioned: the fast kernel keeps them
    assert (np.abs(s.sum(1) - 1.0) <= 1e-5).all()
    gm.close()


@pytest.mark.parametrize("name", ["cfg2_mfcc40_f32.kwsm", "l476_no_yes_f32.kwsm", "l476_no_yes.kwsm", "cfg2_mfcc40_int8.kwsm"])
def test_fast_mode_special_and_golden_clips(name, pkg, oracle):
    """The six known-answer clips and the golden fixtures' clips.  Constant / silent clips have columns whose
    cmvnw output is decided by the reference's own rounding sequence (the "silence canary"): the fast kernel must hand them
    back, and their results are then the exact mode's."""
    import torch
    path = os.path.join(MODELS, name)
    gm = pkg.Model(path, device=0)
    om = OracleModel(oracle, path)
    sp = special_clips()
    g = np.load(os.path.join(GOLDEN, "e2e_l476.npz"))
    gold = np.concatenate([oracle.synth(int(seed), 0, int(g["clips_per_seed"])) for seed in g["seeds"]])
    host = np.concatenate([np.stack(list(sp.values())), gold])
    pcm = torch.from_numpy(host).to("cuda:0")
    s, f, q = run_device(pkg, gm, pkg.MODE_FAST, pcm)
    n_fb = gm.fast_fallback_count()
    se, fe, qe = run_device(pkg, gm, pkg.MODE_EXACT, pcm)
    so, fo, qo = om.run_batch(host, want_features=True)
    names = list(sp)
    for k in ("zeros", "alternating_fullscale", "min"):                   # every frame identical: constant columns
        i = names.index(k)
        assert (bits(f[i]) == bits(fe[i])).all() and (bits(f[i]) == bits(fo[i])).all(), k
        assert (bits(s[i]) == bits(se[i])).all(), k
    assert n_fb >= 3
    if gm.is_float:
        assert np.abs(s - so).max() <= FAST_SCORE_TOL
    else:
        # the network is exact from the int8 tensor on: the oracle's network on the GPU's tensor gives the GPU's scores
        for i in range(len(host)):
            assert (bits(om.dequantize(om.nn_invoke(q[i]))) == bits(s[i])).all(), i
        flips = int((q != qo).sum())
        print("\n%s: %d of %d int8 input values differ from the oracle's on %d clips" % (name, flips, q.size, len(host)))
        assert flips <= q.size // 2000
    gm.close()


@pytest.mark.parametrize("name", ["l476_no_yes.kwsm", "cfg2_mfcc40_int8.kwsm"])
def test_fast_mode_int8_models_flip_rate_and_exact_network(name, pkg, oracle):
    """int8 graphs in fast mode: fast MFCC + the exact int8 network -- since round 3 in the same launch for the two-block
    matrix-core shape (the quantised tensor goes from cmvnw into the network's activation rows in LDS; it only reaches HBM when the
    caller asks for it).  Reported: how many int8 input values land on the other side of a rounding boundary, and how many
    clips' scores change because of it; the scores-only call (one launch, nothing but PCM and scores crosses HBM) must equal the
    call that also returns the feature matrix and the tensor."""
    import torch
    path = os.path.join(MODELS, name)
    gm = pkg.Model(path, device=0)
    om = OracleModel(oracle, path)
    assert gm.fast_is_fused
    B, seed = 8192, 4200
    pcm = torch.empty((B, 16000), dtype=torch.int16, device="cuda:0")
    pkg.synth_clips_device(seed, 0, B, 16000, pcm.data_ptr())
    s, f, q = run_device(pkg, gm, pkg.MODE_FAST, pcm)
    s_only, _, _ = run_device(pkg, gm, pkg.MODE_FAST, pcm, want_f=False)
    assert (bits(s_only) == bits(s)).all()
    so, fo, qo = oracle_all(path, seed, B)
    check_int8_fast_bar(name, om, s, f, q, so, fo, qo)
    gm.close()


def check_int8_fast_bar(name, om, s, f, q, so, fo, qo):
    """The bar of an int8 graph's fast-mode scores, features and input tensors against the reference's (so, fo, qo) for the same clips."""
    flips = (q != qo).sum(axis=1)
    changed = (s != so).any(axis=1)
    print("\n%s fast mode, %d clips: %.4f int8 input flips per clip (%d values per clip), %d clips with a changed score, "
          "max |feature - oracle| = %.3g" % (name, len(s), flips.mean(), q.shape[1], int(changed.sum()), np.abs(f - fo).max()))
    assert np.abs(f - fo).max() <= FAST_FEATURE_TOL
    assert np.abs(q.astype(np.int32) - qo.astype(np.int32)).max() <= 1        # a flip is one quantisation step
    assert flips.mean() <= 0.1 and changed.mean() <= 0.02
    assert not changed[flips == 0].any()                                      # same tensor => same scores, bit for bit
    for i in np.nonzero(changed)[0][:64]:
        assert (bits(om.dequantize(om.nn_invoke(q[i]))) == bits(s[i])).all(), i


def test_fast_mode_ill_conditioned_batch_is_rerun_exactly(pkg, gpu_models=("cfg2_mfcc40_f32.kwsm", "l476_no_yes.kwsm")):
    """A batch made only of constant / silent / repeated-frame clips: every clip is handed back, results are bit-identical to
    KWS_MODE_EXACT."""
    import torch
    rng = np.random.default_rng(5)
    B = 300
    host = np.zeros((B, 16000), np.int16)
    for i in range(B):
        kind = i % 3
        if kind == 1:
            host[i] = rng.integers(-32768, 32767)                              # a constant
        elif kind == 2:
            host[i] = np.tile(rng.integers(-3000, 3000, 320).astype(np.int16), 50)   # every frame the same samples
    pcm = torch.from_numpy(host).to("cuda:0")
    for name in gpu_models:
        gm = pkg.Model(os.path.join(MODELS, name), device=0)
        s, f, q = run_device(pkg, gm, pkg.MODE_FAST, pcm)
        assert gm.fast_fallback_count() == B, name
        se, fe, qe = run_device(pkg, gm, pkg.MODE_EXACT, pcm)
        assert (bits(s) == bits(se)).all() and (bits(f) == bits(fe)).all(), name
        if q is not None:
            assert (q == qe).all()
        gm.close()


def test_fast_mode_edge_batches_and_mode_switch(pkg, oracle):
    import torch
    path = os.path.join(MODELS, "cfg2_mfcc40_f32.kwsm")
    gm = pkg.Model(path, device=0)
    om = OracleModel(oracle, path)
    for n in (1, 3, 65, 2049):                                                  # below / above one clip per wave of the grid
        host = oracle.synth(91, 10 * n, n)
        pcm = torch.from_numpy(host).to("cuda:0")
        s, f, _ = run_device(pkg, gm, pkg.MODE_FAST, pcm)
        so = om.run_batch(host)
        assert np.abs(s - so).max() <= FAST_SCORE_TOL, n
        se, fe, _ = run_device(pkg, gm, pkg.MODE_EXACT, pcm)                    # switching back restores the exact path
        _, feo, _ = om.run_batch(host, want_features=True)
        assert (bits(fe) == bits(feo)).all() and np.abs(se - so).max() <= EXACT_SCORE_TOL, n
    gm.set_mode(pkg.MODE_FAST)
    s = torch.zeros((1, gm.n_labels), dtype=torch.float32, device="cuda:0")
    gm.run_classifier_batch_device(torch.zeros((1, 16000), dtype=torch.int16, device="cuda:0").data_ptr(), 0, s.data_ptr())   # empty batch
    with pytest.raises(pkg.KwsError):
        gm.set_mode(7)
    gm.close()


@pytest.mark.parametrize("name,wps,waves", [("l476_no_yes_f32.kwsm", 3, 12), ("cfg2_mfcc40_f32.kwsm", 3, 11), ("cfg5_dscnn_mfcc40_f32.kwsm", 2, 8)])
def test_three_waves_per_simd_forms(name, wps, waves, pkg, dev_pkg, oracle):
    """Round 6: the float32-network forms exist for two and for three waves per SIMD (csrc/kws_fast.h: KWS_FAST_WPS; the second compilation deals its
    clips out by tickets drawn from a counter in device memory).  Which one a model runs is the plan's choice (kws_fast_tolerance::fused_waves_per_simd);
    whichever it is, a batch's scores do not depend on which wave took which clip: repeated calls -- the ticket counters take turns by launch -- and batch
    sizes around the wave count give the same bits, both builds stay within the fast mode's bar of the oracle, and they agree with each other to the
    arithmetic both share (the cmvnw row groups differ for 40-column matrices: 13 rows per lane against 17)."""
    import torch
    path = os.path.join(MODELS, name)
    gm = pkg.Model(path, device=0)
    tol = gm.fast_tolerance()
    assert (tol["fused_waves_per_simd"], tol["fused_waves"]) == (wps, waves), tol
    om = OracleModel(oracle, path)
    n = 4099                                                                    # not a multiple of either workgroup size
    host = oracle.synth(77, 5, n)
    pcm = torch.from_numpy(host).to("cuda:0")
    so = om.run_batch(host)
    first = None
    for rep in range(5):                                                        # odd and even launch numbers: both ticket counters
        s, _, _ = run_device(pkg, gm, pkg.MODE_FAST, pcm, want_f=False)
        assert np.abs(s - so).max() <= FAST_SCORE_TOL, (name, rep)
        first = s if first is None else first
        assert (bits(s) == bits(first)).all(), (name, rep)
    for m in (1, 7, 11, 12, 13, 255, 256 * waves + 1):                          # fewer clips than waves, one more than a whole round of the grid
        s, _, _ = run_device(pkg, gm, pkg.MODE_FAST, pcm[:m].contiguous(), want_f=False)
        assert (bits(s) == bits(first[:m])).all(), (name, m)
    gm.close()
    if wps == 3:
        # the same model forced onto the other build (development library): both within the bar, and close to each other
        os.environ["KWS_DEV_FAST_WPS"] = "2"
        try:
            g2 = dev_pkg.Model(path, device=0)
        finally:
            del os.environ["KWS_DEV_FAST_WPS"]
        assert g2.fast_tolerance()["fused_waves_per_simd"] == 2
        s2, _, _ = run_device(dev_pkg, g2, dev_pkg.MODE_FAST, pcm, want_f=False)
        assert np.abs(s2 - so).max() <= FAST_SCORE_TOL and np.abs(s2 - first).max() <= 2e-5, name
        g2.close()


def test_fast_mode_depthwise_separable_graph_is_fused_and_extract_mfcc(pkg, oracle):
    """BASELINE configs[4]'s float graph (49x40 MFCC + 7-block depthwise-separable CNN): since round 3 the fast kernel runs it fused
    -- pointwise 1x1 CONV_2D blocks on the matrix cores, DEPTHWISE_CONV_2D taps on the vector ALU, more than four blocks -- so the
    feature matrix never leaves the chip; the extract_mfcc_features entry point follows the mode too."""
    import torch
    path = os.path.join(MODELS, "cfg5_dscnn_mfcc40_f32.kwsm")
    gm = pkg.Model(path, device=0)
    om = OracleModel(oracle, path)
    assert gm.fast_is_fused
    B = 4096
    host = oracle.synth(77, 0, B)
    pcm = torch.from_numpy(host).to("cuda:0")
    # round 4: this graph's logit gain (~42 per unit of rms feature error x sqrt(features); the headline graph: 8) leaves the first tier
    # no room.  Round 5: such a float graph gets the exact kernels' feature matrix (bit for bit) and the fused network on the matrix cores
    # from it (kws_fast_kernel's feat_in form): no clip depends on a cmvnw guard any more
    assert gm.fast_tolerance()["entry_tier"] >= 2
    s, f, _ = run_device(pkg, gm, pkg.MODE_FAST, pcm)
    n_fb = gm.fast_fallback_count()
    s2, _, _ = run_device(pkg, gm, pkg.MODE_FAST, pcm, want_f=False)              # exact cepstra -> cmvnw + fused network: scores
    n_fb2 = gm.fast_fallback_count()
    so, fo, _ = om.run_batch(host, want_features=True)
    print("\ncfg5 fp32 in fast mode (exact features + matrix-core network), %d clips: max |score - oracle| = %.3g, %d clips finished by the exact kernels (%d when only the scores are asked for)"
          % (B, np.abs(s2 - so).max(), n_fb, n_fb2))
    assert np.abs(s - so).max() <= FAST_SCORE_TOL and (bits(f) == bits(fo)).all()
    assert np.abs(s2 - so).max() <= FAST_SCORE_TOL and n_fb2 <= n_fb <= B // 100
    f2 = torch.zeros((B, gm.n_features), dtype=torch.float32, device="cuda:0")
    gm.extract_mfcc_batch_device(pcm.data_ptr(), B, f2.data_ptr())
    torch.cuda.synchronize()
    assert (bits(f2.cpu().numpy()) == bits(f)).all()
    gm.close()


FUSED_DW_GRAPHS = {
    # ("dw", depth_mult, taps, pool, act) / ("pw", out_channels, act) / (out_channels, taps, pool); act 0 none, 1 relu, 3 relu6
    "dscnn_a": dict(seed=21, blocks=((16, 5, 1), ("dw", 1, 3, 1, 1), ("pw", 24, 1), ("dw", 1, 5, 7, 0), ("pw", 8, 3), (8, 3, 7)), n_labels=5),
    "dscnn_b_dw_first_mult2": dict(seed=22, ncep=10, blocks=(("dw", 2, 7, 7, 3), ("pw", 12, 1), ("dw", 1, 3, 7, 1)), n_labels=3),
    "dw_valid_pool_mult2": dict(seed=71, ncep=13, blocks=((12, 3, 1), ("dw", 1, 4, -4, 1), ("pw", 20, 0), ("dw", 2, 2, 4, 3), ("pw", 6, 1)), n_labels=4),
    "dw_same_pool_ragged": dict(seed=74, ncep=13, blocks=((12, 3, 1), ("dw", 1, 3, 2, 1), ("pw", 10, 1), ("dw", 1, 9, 1, 0), ("pw", 6, 1)), n_labels=4),   # 49 -> 25 (ragged), nine taps
    "dw40": dict(seed=72, num_filters=40, ncep=40, low=300, high=0, blocks=(("dw", 1, 5, 1, 1), ("pw", 32, 1), ("dw", 1, 3, 7, 1), ("pw", 16, 3), (8, 3, 7)), n_labels=6),
    "eight_blocks": dict(seed=73, ncep=13, blocks=((16, 3, 1), ("dw", 1, 3, 1, 1), ("pw", 16, 1), ("dw", 1, 3, 2, 1), ("pw", 16, 1), ("dw", 1, 3, 2, 1), ("pw", 16, 1), ("dw", 1, 3, 7, 0)), n_labels=4),
}


@pytest.mark.parametrize("key", sorted(FUSED_DW_GRAPHS))
def test_fast_mode_fused_depthwise_separable_graphs(key, dev_pkg, oracle, tmp_path, monkeypatch):
    """Depthwise-separable float graphs in the fused fast kernel: depthwise first block, depth multiplier 2, VALID pooling with a
    dropped tail, ragged SAME windows, 40-channel inputs, eight blocks -- each against the restated float kernels
    (reference/depthwiseconv_float.h:25, reference/conv.h:28-99) within the fast mode's score tolerance, incl. the special clips."""
    import sys
    import torch
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from dequantize_model import dequantize
    from kws_testlib import synth_model_blob
    blob = dequantize(synth_model_blob(**FUSED_DW_GRAPHS[key]))
    # these random-weight graphs have whatever logit gain their draws gave them: most would be routed past the first tier (round 4).  This
    # test is about the fused kernel's arithmetic: start every batch call in it (the guards still decide which clips it keeps) -- a
    # development switch, so the development build of the library (conftest.py: dev_pkg)
    pkg = dev_pkg
    monkeypatch.setenv("KWS_DEV_FAST_ENTRY", "1")
    p = tmp_path / ("%s.kwsm" % key)
    p.write_bytes(blob)
    om = OracleModel(oracle, str(p))
    gm = pkg.Model(blob=blob)
    gm.set_mode(pkg.MODE_FAST)
    assert gm.fast_is_fused, key
    if key.startswith("w3_"):
        assert gm.fast_tolerance()["fused_waves_per_simd"] == 3, (key, gm.fast_tolerance())          # the build these graphs are here for
    B = 700
    host = np.concatenate([oracle.synth(400 + len(key), 5, B - 6), np.stack(list(special_clips().values()))[:6]])
    pcm = torch.from_numpy(np.ascontiguousarray(host)).to("cuda:0")
    s, f, _ = run_device(pkg, gm, pkg.MODE_FAST, pcm)
    so, fo, _ = om.run_batch(host, want_features=True)
    assert np.abs(s - so).max() <= FAST_SCORE_TOL, (key, float(np.abs(s - so).max()))
    se, _, _ = run_device(pkg, gm, pkg.MODE_EXACT, pcm)
    assert np.abs(se - so).max() <= EXACT_SCORE_TOL, key
    gm.close()


def test_fast_mode_random_mfcc_configurations(pkg, oracle):
    """The random DSP configurations of the exact-mode fuzz test (32 / 40 filters, 2..40 cepstra, cmvnw windows 13..137, filterbank
    ranges) through the fast kernel: features within tolerance of the restatement, or bit-identical where the clip was handed
    back; configurations outside the fast kernel are refused by kws_set_mode with KWS_ERROR_UNSUPPORTED_MODEL."""
    import torch
    from kws_testlib import L476_CONFIG, random_dsp_spec, synth_model_blob
    clips = oracle.synth(21, 0, 24)
    pcm = torch.from_numpy(clips).to("cuda:0")
    n_ok = n_refused = 0
    worst = 0.0
    for seed in range(40):
        cfg_kw, blob_kw = random_dsp_spec(seed)
        try:
            gm = pkg.Model(blob=synth_model_blob(**blob_kw))
        except pkg.KwsError as e:
            assert e.code == -18
            continue
        try:
            gm.set_mode(pkg.MODE_FAST)
        except pkg.KwsError as e:
            assert e.code == -18, (seed, cfg_kw)
            n_refused += 1
            gm.close()
            continue
        cfg = L476_CONFIG().copy(**cfg_kw)
        _, f, _ = run_device(pkg, gm, pkg.MODE_FAST, pcm)
        fo = np.stack([oracle.extract_mfcc(c, cfg) for c in clips])
        worst = max(worst, float(np.abs(f - fo).max()))
        assert np.abs(f - fo).max() <= FAST_FEATURE_TOL, (seed, cfg_kw)
        gm.close()
        n_ok += 1
    print("\nfast mode over %d random MFCC configurations (%d outside the fast kernel): max |feature - oracle| = %.3g" % (n_ok, n_refused, worst))
    assert n_ok >= 25, (n_ok, n_refused)


@pytest.mark.parametrize("name,mode", [("cfg5_dscnn_mfcc40_int8.kwsm", "exact"), ("cfg5_dscnn_mfcc40_f32.kwsm", "exact"),
                                       ("cfg5_dscnn_mfcc40_int8.kwsm", "fast"), ("cfg2_mfcc40_f32.kwsm", "fast")])
def test_full_size_properties_other_workloads(name, mode, pkg, oracle):
    """BASELINE configs[4]'s model (49x40 MFCC + 7-block depthwise-separable CNN, 12 labels) and the fast mode of the headline
    graph at the full 65 536 clips: (a) permuting the batch permutes the scores bit for bit, (b) duplicated clips give identical
    rows, (c) a strided sample of rows equals the oracle (exact mode: int8 bit for bit, float within 1e-6; fast mode: within 1e-4 /
    the int8 network exact on the GPU's own tensor), (d) rows are softmaxes."""
    import torch
    path = os.path.join(MODELS, name)
    gm = pkg.Model(path, device=0)
    om = OracleModel(oracle, path)
    gm.set_mode(pkg.MODE_FAST if mode == "fast" else pkg.MODE_EXACT)
    B, C = 65536, gm.n_labels
    pcm = torch.empty((B, 16000), dtype=torch.int16, device="cuda:0")
    pkg.synth_clips_device(0, 0, B, 16000, pcm.data_ptr())
    pcm[1::4096] = pcm[0::4096]
    scores = torch.empty((B, C), dtype=torch.float32, device="cuda:0")
    gm.run_classifier_batch_device(pcm.data_ptr(), B, scores.data_ptr())
    torch.cuda.synchronize()
    s = scores.cpu().numpy()
    assert (s[1::4096] == s[0::4096]).all()                                                  # (b)
    perm = torch.randperm(B, device="cuda:0", generator=torch.Generator(device="cuda:0").manual_seed(3))
    pcm2 = pcm[perm].contiguous()
    scores2 = torch.empty_like(scores)
    gm.run_classifier_batch_device(pcm2.data_ptr(), B, scores2.data_ptr())
    torch.cuda.synchronize()
    assert torch.equal(scores2, scores[perm])                                                # (a)
    idx = np.arange(5, B, 2731)
    host = pcm[torch.from_numpy(idx).cuda()].cpu().numpy()
    so = om.run_batch(host)
    if gm.is_float:
        assert np.abs(s[idx] - so).max() <= (FAST_SCORE_TOL if mode == "fast" else EXACT_SCORE_TOL)      # (c)
        assert (np.abs(s.sum(1) - 1.0) <= 1e-5).all()                                        # (d)
    elif mode == "exact":
        assert (bits(s[idx]) == bits(so)).all()
    else:
        assert (s[idx] != so).any(axis=1).mean() <= 0.05                                     # a few clips: an input value on a rounding boundary
    if not gm.is_float:
        assert (np.abs(s * 256 - np.round(s * 256)) == 0).all() and (np.abs(s.sum(1) - 1.0) <= 8 / 256).all()
    gm.close()


@pytest.mark.parametrize("name", ["cfg2_mfcc40_f32.kwsm", "l476_no_yes_f32.kwsm", "l476_no_yes.kwsm", "cfg2_mfcc40_int8.kwsm"])
def test_fast_mode_streams_follow_the_continuous_oracle(name, pkg, oracle):
    """kws_streams_step_device in KWS_MODE_FAST: the slice's MFCC is exact, the whole-window cmvnw + network go through the fast
    kernel reading the ring-indexed rolling buffers.  Float graphs: every score within 1e-4 of the restated
    run_classifier_continuous(); int8 graphs: scores on the output grid, at most a few of them one step away.  Includes streams
    of silence and DC (constant columns -> guard -> exact re-run) and a run_classifier_init() in the middle."""
    import torch
    from kws_testlib import OracleContinuous
    path = os.path.join(MODELS, name)
    gm = pkg.Model(path, device=0)
    om = OracleModel(oracle, path)
    gm.set_mode(pkg.MODE_FAST)
    S = 24
    audio = oracle.synth(31, 0, S * 3).reshape(S, 3 * 16000).copy()
    audio[0] = 0
    audio[1] = 1234
    audio[2, 20000:] = 0                                                  # goes silent mid-stream
    sb = pkg.StreamBatch(gm, S)
    ocs = [OracleContinuous(om) for _ in range(S)]
    for oc in ocs:
        oc.init()
    scores = torch.empty((S, gm.n_labels), dtype=torch.float32, device="cuda")
    n_prod = n_diff = 0
    worst = 0.0
    for phase in range(2):
        for k in range(11 if phase == 0 else 6):
            sl = np.ascontiguousarray(audio[:, k * 4000:(k + 1) * 4000])
            d = torch.from_numpy(sl).cuda()
            produced = sb.step_device(d.data_ptr(), 4000, scores.data_ptr())
            torch.cuda.synchronize()
            got = scores.cpu().numpy()
            for s in range(S):
                rc, p, want = ocs[s].step(sl[s])
                assert rc == 0 and p == produced, (name, phase, k, s)
                if not p:
                    continue
                n_prod += 1
                err = float(np.abs(got[s] - want).max())
                worst = max(worst, err)
                if gm.is_float:
                    assert err <= FAST_SCORE_TOL, (name, phase, k, s, err)
                else:
                    n_diff += int(err > 0)
                    assert err <= 2.5 / 256, (name, phase, k, s, err)
                if s == 0:                                               # silence: constant columns -> exact path
                    tol = 1e-6 if gm.is_float else 0.0
                    assert err <= tol, (name, phase, k, s, err)
        sb.init()
        for oc in ocs:
            oc.init()
    assert n_prod > 100
    if not gm.is_float:
        assert n_diff <= max(2, n_prod // 50), (name, n_diff, n_prod)
    assert gm.fast_fallback_count() >= 1                                  # last step: at least the silent stream
    sb.close()
    gm.close()


FUSED_POOL_GRAPHS = {
    # (out_channels, taps, pool): positive pool = SAME (a ragged last window is clipped), negative = VALID (the tail is dropped)
    "pool7_7": dict(seed=61, ncep=13, blocks=((30, 7, 7), (10, 7, 7)), n_labels=4),                  # the shipped shape
    "pool5_valid_one_block": dict(seed=62, ncep=13, blocks=((24, 5, -5),), n_labels=5),                # 49 -> 9 (rows 45..48 dropped), Dense over 216
    "pool4_valid": dict(seed=63, ncep=16, blocks=((16, 3, -4), (8, 3, -4)), n_labels=3),               # 49 -> 12 (row 48 dropped) -> 3
    "pool6_valid_40ch": dict(seed=64, num_filters=40, ncep=40, low=300, high=0, blocks=((32, 3, -6), (16, 3, 1)), n_labels=6),   # 49 -> 8
    "pool2_small_windows": dict(seed=65, ncep=13, blocks=((8, 3, 2), (16, 3, 2)), n_labels=4),         # windows < 4 rows: staging path
    "pool8_valid_then_none": dict(seed=66, ncep=20, blocks=((12, 4, -8), (12, 2, 1)), n_labels=4),     # 49 -> 6 (row 48 dropped), then an un-pooled block
    # round 6, the three-waves-per-SIMD build: first blocks whose fragments come from L2 (40 filters: the LDS block has no room) in k-step counts that are
    # not multiples of three -- the rotating-set contraction loop walks whole trips of three, the steps past the last one multiply the zero block
    "w3_l2_fragments_7_ksteps": dict(seed=67, num_filters=40, ncep=40, low=300, high=0, blocks=((30, 5, 7), (10, 5, 7)), n_labels=4),    # 5 taps x 5 groups = 25 -> 7 k-steps
    "w3_l2_fragments_5_ksteps": dict(seed=68, num_filters=40, ncep=40, low=300, high=0, blocks=((24, 4, 7), (12, 3, 7)), n_labels=5),    # 4 taps x 5 groups = 20 -> 5 k-steps
}


@pytest.mark.parametrize("key", sorted(FUSED_POOL_GRAPHS))
def test_fast_mode_fused_graphs_with_other_pooling_shapes(key, pkg, oracle, tmp_path):
    """The fused float network of kws_fast_kernel over pooling shapes other than the shipped 7 / 7: windows taken on the raw
    accumulators (non-overlapping, >= 4 rows: SAME with a ragged last window, VALID with a dropped tail) and the staging path
    (windows of 2 or 3 rows), each against the restated float kernels within the fast mode's score tolerance."""
    import sys
    import torch
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from dequantize_model import dequantize
    from kws_testlib import synth_model_blob
    blob = dequantize(synth_model_blob(**FUSED_POOL_GRAPHS[key]))
    p = tmp_path / ("%s.kwsm" % key)
    p.write_bytes(blob)
    om = OracleModel(oracle, str(p))
    try:
        gm = pkg.Model(blob=blob)
    except pkg.KwsError as e:                       # a draw outside the documented limits of the plan builder
        assert e.code == -18
        pytest.skip("graph outside the kernels' limits: %s" % e)
    gm.set_mode(pkg.MODE_FAST)
    assert gm.fast_is_fused, key
    B = 700
    host = np.concatenate([oracle.synth(300 + len(key), 5, B - 6), np.stack(list(special_clips().values()))[:6]])
    pcm = torch.from_numpy(np.ascontiguousarray(host)).to("cuda:0")
    s, f, _ = run_device(pkg, gm, pkg.MODE_FAST, pcm)
    so, fo, _ = om.run_batch(host, want_features=True)
    assert np.abs(s - so).max() <= FAST_SCORE_TOL, (key, float(np.abs(s - so).max()))
    gm.close()


@pytest.mark.parametrize("factor", [1.0e-4, 3.0e3])
def test_split_operand_contraction_over_the_scale_range(factor, pkg, tmp_path):
    """Round 5: the fused network's CONV_2D blocks run on v_mfma_f32_16x16x32_f16 with every fp32 operand carried as two halves of x * 2^k
    (kws_fast.hip: fast_split_image; k from the image's largest magnitude per clip, the weights' k per block on the host).  The scaling is
    what keeps the halves inside binary16's range: the headline graph with its first convolution x 1e-4 (activations of ~1e-4 behind it)
    and x 3e3 (activations of several thousand, logits of +-1e4) must come out with the LOGITS of the reference's float kernels to fp32
    accuracy -- relative to the largest logit, the yardstick a sum of products rounds against."""
    import sys
    import torch
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from test_gain_calibration import scaled_first_conv
    path = str(tmp_path / "cfg2_conv1_scaled.kwsm")
    scaled_first_conv(os.path.join(MODELS, "cfg2_mfcc40_f32.kwsm"), factor, path)
    B, seed = 1024, 31
    pcm = torch.empty((B, 16000), dtype=torch.int16, device="cuda:0")
    pkg.synth_clips_device(seed, 0, B, 16000, pcm.data_ptr())
    gm = pkg.Model(path, device=0)
    assert gm.fast_is_fused
    z_t = torch.zeros((B, gm.n_labels), dtype=torch.float32, device="cuda:0")
    gm.set_logits_tap(z_t.data_ptr())
    s, f, _ = run_device(pkg, gm, pkg.MODE_FAST, pcm, want_f=False)
    gm.set_logits_tap(None)
    so, fo, _, zo = oracle_all(path, seed, B, want_logits=True)
    z = z_t.cpu().numpy()
    rel = float(np.abs(z.astype(np.float64) - zo).max() / max(1.0, float(np.abs(zo).max())))
    print("\nfirst convolution x %g: entry tier %d, max |logit| %.3g, max |logit - oracle| / max |logit| = %.3g, max |score - oracle| = %.3g"
          % (factor, gm.fast_tolerance()["entry_tier"], float(np.abs(zo).max()), rel, float(np.abs(s - so).max())))
    assert not np.isnan(s).any() and np.abs(s - so).max() <= FAST_SCORE_TOL
    assert rel <= 2.0e-5
    gm.close()


def test_fast_mode_guard_follows_the_model_gain(pkg, oracle, tmp_path):
    """a deliberately high-gain model (the headline graph with its first convolution's weights x 8).  The
    library must measure the higher gain at kws_create, tighten the guard with it -- the same clips that the base model keeps in the
    fast kernel are now handed on --, and the 1e-4 score bar must still hold for every clip; the clips a fast tier did keep have their
    logit differences within the bar stated at the logits."""
    import sys
    import torch
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from test_gain_calibration import scaled_first_conv
    base = os.path.join(MODELS, "cfg2_mfcc40_f32.kwsm")
    hot = str(tmp_path / "cfg2_conv1_x8.kwsm")
    scaled_first_conv(base, 8.0, hot)
    B, seed = 4096, 77
    pcm = torch.empty((B, 16000), dtype=torch.int16, device="cuda:0")
    pkg.synth_clips_device(seed, 0, B, 16000, pcm.data_ptr())
    res = {}
    for tag, path in (("base", base), ("hot", hot)):
        gm = pkg.Model(path, device=0)
        tol = gm.fast_tolerance()
        z_t = torch.zeros((B, gm.n_labels), dtype=torch.float32, device="cuda:0")
        gm.set_logits_tap(z_t.data_ptr())
        s, f, _ = run_device(pkg, gm, pkg.MODE_FAST, pcm)
        n_t2, n_ex = gm.fast_fallback_count(), gm.fast_exact_count()
        se, fe, _ = run_device(pkg, gm, pkg.MODE_EXACT, pcm)
        gm.set_logits_tap(None)
        so, fo, _, zo = oracle_all(path, seed, B, want_logits=True)
        exact = (bits(f) == bits(fe)).all(axis=1)
        res[tag] = dict(gain=tol["total_gain"], tol=tol["uniform_feature_tol"], entry=tol["entry_tier"], t2=n_t2, ex=n_ex, ds=float(np.abs(s - so).max()),
                        dz=float(pair_error(z_t.cpu().numpy(), zo)[~exact].max(initial=0.0)), pq=float(np.median((so * (1 - so)).max(axis=1))))
        assert (bits(fe) == bits(fo)).all()
        assert res[tag]["ds"] <= FAST_SCORE_TOL, res
        if res[tag]["entry"] == 1:
            assert (bits(s[exact]) == bits(se[exact])).all()            # a clip the exact kernels finished carries their bits
        else:
            # round 5: a float graph whose gain leaves the fast DSP tiers no room gets the exact kernels' feature matrix for EVERY clip (bit for
            # bit) and the network on the matrix cores from it: the scores are the exact mode's up to the network's own arithmetic
            assert exact.all() and np.abs(s - se).max() <= FAST_SCORE_TOL / 2      # (measured 2.7e-5 for the x 8 graph, whose logits reach +-45)
        gm.close()
    print("\nfirst convolution x 8 on %d clips: %s" % (B, res))
    assert 5.0 <= res["hot"]["gain"] / res["base"]["gain"] <= 12.0
    assert res["hot"]["tol"] <= res["base"]["tol"] / 5.0
    # the base model starts in the fast kernel and keeps the bench's clips there; the hot one's gain leaves the first tier no room: its
    # batch calls start from the exact kernels' cepstra (or run the exact kernels throughout)
    assert res["base"]["entry"] == 1 and res["base"]["t2"] <= B // 50
    assert res["hot"]["entry"] >= 2
