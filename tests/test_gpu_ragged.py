"""-m gpu: kws_run_classifier_ragged_device -- run_classifier() for a batch of clips of their own lengths (include/kws/kws.h).

Expected values are the reference's own where a fixture holds them (tests/golden/other_length_l476.npz, mfe_other_length_l432.npz) and the
oracle's functions composed as tests/test_other_window_length.py composes them everywhere else: extract_mfcc / extract_mfe of clip[:L],
zero-extended to the feature count, then quantize_input / run_inference.  int8 graphs and every feature matrix: bit for bit; float32 scores:
within 1e-6 (the bars of the other entry points).  Output buffers are prefilled with 0xFF bytes: the call has to write the zeros itself."""
import os

import numpy as np
import pytest

from kws_testlib import GOLDEN, MODELS, ROOT, OracleModel, bits, synth_model_blob

pytestmark = pytest.mark.gpu
BAD_ARGUMENT, UNSUPPORTED_MODEL = -20, -18
STRIDE, FLEN = 320, 320            # the shipped impulse's frames: 20 ms every 20 ms at 16 kHz


@pytest.fixture(scope="module")
def pkg():
    import sys
    sys.path.insert(0, ROOT)
    import torch  # noqa: F401
    from __graft_entry__ import load_package
    return load_package()


def _pack(clips, gaps=None, seed=0):
    """the clips back to back (gaps[i] samples of noise in front of clip i): buffer, offsets, lengths"""
    gaps = [0] * len(clips) if gaps is None else gaps
    total = sum(len(c) for c in clips) + sum(gaps) + 16
    buf = np.random.default_rng(seed).integers(-32768, 32768, total, dtype=np.int16)
    offs, at = [], 0
    for c, g in zip(clips, gaps):
        at += g
        buf[at:at + len(c)] = c
        offs.append(at)
        at += len(c)
    return buf, np.array(offs, np.uint64), np.array([len(c) for c in clips], np.uint64)


def _device(buf):
    import torch
    return torch.from_numpy(np.ascontiguousarray(buf)).to("cuda:0")


def _run(m, d_pcm, offs, lens, want=("s", "f", "q")):
    """one ragged call into buffers prefilled with 0xFF bytes -> dict of numpy arrays"""
    import torch
    B = len(lens)
    shape = {"s": (B, m.n_labels * 4), "f": (B, m.n_features * 4), "q": (B, m.n_features)}
    t = {k: torch.full(shape[k], 0xFF, dtype=torch.uint8, device="cuda:0") for k in want if not (k == "q" and m.is_float)}
    ptr = lambda k: t[k].data_ptr() if k in t else None
    m.run_classifier_ragged_device(d_pcm.data_ptr(), offs, lens, ptr("s"), ptr("f"), ptr("q"))
    torch.cuda.synchronize()
    out = {k: v.cpu().numpy() for k, v in t.items()}
    for k in ("s", "f"):
        if k in out:
            out[k] = out[k].view(np.float32)
    if "q" in out:
        out["q"] = out["q"].view(np.int8)
    return out


def _compose(oracle, om, clip, cfg=None, mfe=False):
    """the oracle composition: features (zero-extended), q, scores of one clip of its own length"""
    cfg = cfg or om.cfg
    f = oracle.extract_mfe(clip, cfg) if mfe else oracle.extract_mfcc(clip, cfg)
    padded = np.zeros(om.n_features, np.float32)
    padded[:f.size] = f
    return padded, om.quantize_input(padded), om.run_inference(padded)


def _check_rows(m, out, want, rows=None, what=""):
    """want: list of (features, q, scores) per row of `rows` (default: all)"""
    rows = range(len(want)) if rows is None else rows
    for r, (f, q, s) in zip(rows, want):
        assert (bits(out["f"][r]) == bits(f)).all(), (what, r, "features")
        if m.is_float:
            assert np.abs(out["s"][r] - s).max() <= 1e-6, (what, r, "scores")
        else:
            assert (out["q"][r] == q).all(), (what, r, "q")
            assert (bits(out["s"][r]) == bits(s)).all(), (what, r, "scores")


# ---- 1. the reference's own bits, MFCC block ------------------------------------------------------------------------------------------
def test_ragged_matches_the_reference_fixture_mfcc(pkg, oracle):
    g = np.load(os.path.join(GOLDEN, "other_length_l476.npz"))
    order = [(i, j) for i in range(len(g["clips"])) for j in range(len(g["lengths"]))]
    np.random.default_rng(476).shuffle(order)
    assert len(order) == 33
    buf, offs, lens = _pack([g["clips"][i][:g["lengths"][j]] for i, j in order])
    assert (offs % 2 == 1).any() and (offs % 8 != 0).any()           # odd offsets included
    d = _device(buf)
    for name, key in (("l476_no_yes.kwsm", "scores"), ("l476_no_yes_f32.kwsm", "twin_scores")):
        m = pkg.Model(os.path.join(MODELS, name), device=0)
        om = OracleModel(oracle, os.path.join(MODELS, name))
        out = _run(m, d, offs, lens)
        for r, (i, j) in enumerate(order):
            assert (bits(out["f"][r]) == bits(g["features"][i, j])).all(), (name, i, int(g["lengths"][j]))
            if m.is_float:
                assert np.abs(out["s"][r] - g[key][i, j]).max() <= 1e-6, (name, i, int(g["lengths"][j]))
            else:
                assert (bits(out["s"][r]) == bits(g[key][i, j])).all(), (name, i, int(g["lengths"][j]))
                assert (out["q"][r] == om.quantize_input(g["features"][i, j])).all(), (name, i, int(g["lengths"][j]))
        m.close()


# ---- 2. the reference's own bits, MFE block -------------------------------------------------------------------------------------------
def test_ragged_matches_the_reference_fixture_mfe(pkg):
    from test_other_window_length import _mfe_blob
    g = np.load(os.path.join(GOLDEN, "mfe_other_length_l432.npz"))
    order = [(i, j) for i in range(len(g["clips"])) for j in range(len(g["lengths"]))]
    np.random.default_rng(432).shuffle(order)
    assert len(order) == 27
    buf, offs, lens = _pack([g["clips"][i][:g["lengths"][j]] for i, j in order])
    m = pkg.Model(blob=_mfe_blob())
    out = _run(m, _device(buf), offs, lens)
    for r, (i, j) in enumerate(order):
        assert (bits(out["f"][r]) == bits(g["features"][i, j])).all(), (i, int(g["lengths"][j]))
        assert (out["q"][r] == g["q"][i, j]).all(), (i, int(g["lengths"][j]))
        assert (bits(out["s"][r]) == bits(g["scores"][i, j])).all(), (i, int(g["lengths"][j]))
    m.close()


# ---- 3. every frame count, both ends of its length range ------------------------------------------------------------------------------
def _edge_lengths(nf=49, clip=16000):
    return [L for n in range(1, nf + 1) for L in (FLEN + STRIDE * n, FLEN + STRIDE * n + STRIDE - 1)] + [clip]


@pytest.fixture(scope="module")
def edge_clips(oracle):
    lens = _edge_lengths()
    pool = oracle.synth(31, 0, len(lens), 16319)
    return [pool[k][:L] for k, L in enumerate(lens)]


@pytest.mark.parametrize("name", ["l476_no_yes.kwsm", "cfg2_mfcc40_int8.kwsm", "cfg2_mfcc40_f32.kwsm"])
def test_ragged_every_frame_count_at_both_ends(name, pkg, oracle, edge_clips):
    m = pkg.Model(os.path.join(MODELS, name), device=0)
    om = OracleModel(oracle, os.path.join(MODELS, name))
    assert m.n_frames == 49 and m.clip_samples == 16000
    assert [m.window_frame_count(len(c)) for c in edge_clips] == [n for n in range(1, 50) for _ in (0, 1)] + [49]
    buf, offs, lens = _pack(edge_clips)
    out = _run(m, _device(buf), offs, lens)
    _check_rows(m, out, [_compose(oracle, om, c) for c in edge_clips], what=name)
    m.close()


# ---- 4. agreement with the fixed-length call ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["l476_no_yes.kwsm", "cfg2_mfcc40_f32.kwsm"])
def test_ragged_full_length_clips_equal_the_batch_call(name, pkg, oracle):
    import torch
    B = 600
    m = pkg.Model(os.path.join(MODELS, name), device=0)
    n = m.clip_samples
    d = _device(oracle.synth(44, 0, B, n))
    s = torch.zeros((B, m.n_labels), dtype=torch.float32, device="cuda:0")
    f = torch.zeros((B, m.n_features), dtype=torch.float32, device="cuda:0")
    q = None if m.is_float else torch.zeros((B, m.n_features), dtype=torch.int8, device="cuda:0")
    m.run_classifier_batch_device(d.data_ptr(), B, s.data_ptr(), f.data_ptr(), None if q is None else q.data_ptr())
    torch.cuda.synchronize()
    offs, lens = np.arange(B, dtype=np.uint64) * n, np.full(B, n, np.uint64)

    def same(out):
        assert (bits(out["s"]) == bits(s.cpu().numpy())).all() and (bits(out["f"]) == bits(f.cpu().numpy())).all()
        assert m.is_float or (out["q"] == q.cpu().numpy()).all()
    same(_run(m, d, offs, lens))
    # with the handle in KWS_MODE_FAST: still the exact bits, and the mode and both counters are what they were
    m.set_mode(pkg.MODE_FAST)
    m.run_classifier_batch_device(d.data_ptr(), B, torch.empty_like(s).data_ptr(), None)
    torch.cuda.synchronize()
    before = (m.L.kws_get_mode(m.h), m.fast_fallback_count(), m.fast_exact_count())
    same(_run(m, d, offs, lens))
    assert (m.L.kws_get_mode(m.h), m.fast_fallback_count(), m.fast_exact_count()) == before and before[0] == pkg.MODE_FAST
    m.close()


# ---- 5. more clips than resident waves, and isolation ---------------------------------------------------------------------------------
def test_ragged_many_clips_isolated_from_each_other_and_from_what_surrounds_them(pkg, oracle):
    B = 5000
    rng = np.random.default_rng(5000)
    m = pkg.Model(os.path.join(MODELS, "l476_no_yes.kwsm"), device=0)
    om = OracleModel(oracle, os.path.join(MODELS, "l476_no_yes.kwsm"))
    nfr = (np.arange(B) % 49) + 1                                   # all frame counts, cycling ...
    rng.shuffle(nfr)                                                # ... in a seeded shuffle
    lens_i = FLEN + STRIDE * nfr + rng.integers(0, STRIDE, B)
    pool = oracle.synth(55, 0, 64, 16319)
    clips = [pool[k % 64][:L] for k, L in enumerate(lens_i)]
    gaps = rng.integers(0, 12, B).tolist()
    buf, offs, lens = _pack(clips, gaps, seed=1)
    out = _run(m, _device(buf), offs, lens)
    # every value behind a row's fitting part is +0.0 (q: quantise(0))
    qz = om.quantize_input(np.zeros(om.n_features, np.float32))[0]
    col = np.arange(m.n_features)[None, :] >= (13 * nfr)[:, None]
    assert (bits(out["f"])[col] == 0).all() and (out["q"][col] == qz).all()
    assert all((bits(out["f"][r, :13 * nfr[r]]) != 0).any() for r in range(0, B, 97))
    # a fixed sample of 64 rows equals the same clip submitted alone
    for r in np.random.default_rng(64).choice(B, 64, replace=False):
        one = _run(m, _device(np.concatenate([clips[r], np.zeros(8, np.int16)])), np.zeros(1, np.uint64), lens[r:r + 1])
        assert all((bits(one[k][0]) == bits(out[k][r])).all() for k in ("s", "f")) and (one["q"][0] == out["q"][r]).all(), r
    # a strided sample of 200 rows equals the oracle composition
    rows = range(0, B, 25)
    _check_rows(m, out, [_compose(oracle, om, clips[r]) for r in rows], rows=rows, what="strided")
    # other garbage between and around the clips: identical bits
    buf2, offs2, _ = _pack(clips, gaps, seed=2)
    assert (offs2 == offs).all() and (buf2 != buf).any()
    out2 = _run(m, _device(buf2), offs, lens)
    assert all((bits(out2[k]) == bits(out[k])).all() for k in ("s", "f")) and (out2["q"] == out["q"]).all()
    # the clips in reverse order: the rows in reverse order
    out3 = _run(m, _device(buf), offs[::-1].copy(), lens[::-1].copy())
    assert all((bits(out3[k]) == bits(out[k][::-1])).all() for k in ("s", "f")) and (out3["q"] == out["q"][::-1]).all()
    m.close()


# ---- 6. offsets and overlap -----------------------------------------------------------------------------------------------------------
def test_ragged_any_offset_and_overlapping_clips(pkg, oracle):
    m = pkg.Model(os.path.join(MODELS, "l476_no_yes.kwsm"), device=0)
    om = OracleModel(oracle, os.path.join(MODELS, "l476_no_yes.kwsm"))
    clip = oracle.synth(66, 0, 1, 16319)[0][:9001]
    buf, offs, lens = _pack([clip] * 9)                  # 9001 = 1 (mod 8): back to back, copy k starts at an offset = k (mod 8)
    assert (offs % 8 == np.array([0, 1, 2, 3, 4, 5, 6, 7, 0])).all()
    out = _run(m, _device(buf), offs, lens)
    want = _compose(oracle, om, clip)
    _check_rows(m, out, [want] * 9, what="offsets")
    # two entries over the same start with different lengths: other wrap samples, other features
    pool = oracle.synth(67, 0, 1, 16319)[0]
    offs2, lens2 = np.array([3, 3, 3], np.uint64), np.array([15681, 15999, 15680], np.uint64)
    out = _run(m, _device(np.concatenate([np.zeros(3, np.int16), pool])), offs2, lens2)
    _check_rows(m, out, [_compose(oracle, om, pool[:int(L)]) for L in lens2], what="overlap")
    assert (bits(out["f"][0]) != bits(out["f"][1])).any() and (bits(out["f"][0]) != bits(out["f"][2])).any()
    m.close()


# ---- 7. refusals on the device path ---------------------------------------------------------------------------------------------------
def test_ragged_refusals_leave_the_outputs_untouched(pkg, oracle, edge_clips):
    import torch
    m = pkg.Model(os.path.join(MODELS, "l476_no_yes.kwsm"), device=0)
    om = OracleModel(oracle, os.path.join(MODELS, "l476_no_yes.kwsm"))
    d = _device(oracle.synth(77, 0, 8, 16384).reshape(-1))
    offs = np.arange(7, dtype=np.uint64) * 16384
    for bad in (0, 639, 16320):
        lens = np.full(7, 8000, np.uint64)
        lens[3] = bad
        t = {k: torch.full((7, w), 0xFF, dtype=torch.uint8, device="cuda:0") for k, w in (("s", 4 * m.n_labels), ("f", 4 * m.n_features), ("q", m.n_features))}
        with pytest.raises(pkg.KwsError) as e:
            m.run_classifier_ragged_device(d.data_ptr(), offs, lens, t["s"].data_ptr(), t["f"].data_ptr(), t["q"].data_ptr())
        torch.cuda.synchronize()
        assert e.value.code == BAD_ARGUMENT and "clip 3 " in str(e.value) and "%d samples" % bad in str(e.value), str(e.value)
        assert all((v.cpu().numpy() == 0xFF).all() for v in t.values())
    lens = np.full(7, 8000, np.uint64)
    with pytest.raises(pkg.KwsError) as e:
        m.run_classifier_ragged_device(d.data_ptr(), offs, lens, None, None, None)
    assert e.value.code == BAD_ARGUMENT
    s = torch.full((7, 4 * m.n_labels), 0xFF, dtype=torch.uint8, device="cuda:0")
    m.run_classifier_ragged_device(d.data_ptr(), offs[:0], lens[:0], s.data_ptr())         # B = 0: OK, nothing written
    m.run_classifier_ragged_device(None, offs[:0], lens[:0], s.data_ptr())
    torch.cuda.synchronize()
    assert (s.cpu().numpy() == 0xFF).all()
    mf = pkg.Model(os.path.join(MODELS, "l476_no_yes_f32.kwsm"), device=0)
    with pytest.raises(pkg.KwsError) as e:
        mf.run_classifier_ragged_device(d.data_ptr(), offs, lens, s.data_ptr(), None, s.data_ptr())
    assert e.value.code == UNSUPPORTED_MODEL                                                  # as kws_run_classifier_batch_device refuses it
    mf.close()
    # scores == NULL: a ragged extract_mfcc_features
    ten = edge_clips[:10]
    buf, offs, lens = _pack(ten)
    out = _run(m, _device(buf), offs, lens, want=("f",))
    for r, c in enumerate(ten):
        assert (bits(out["f"][r]) == bits(_compose(oracle, om, c)[0])).all(), r
    m.close()


# ---- 8. a general-shape plan ----------------------------------------------------------------------------------------------------------
def test_ragged_general_shape_plan(pkg, oracle, tmp_path):
    blob = synth_model_blob(seed=3, blocks=((8, 3, 7), (4, 3, 7)), n_labels=3, fft_length=512)
    path = str(tmp_path / "m.kwsm")
    open(path, "wb").write(blob)
    om = OracleModel(oracle, path)
    m = pkg.Model(blob=blob)
    assert m.mfcc_kernel in ("kws_spectral_lds_kernel", "kws_spectral_generic_kernel")
    lens = [640, 959, 960, 1283, 4000, 4001, 7777, 8000, 12345, 15999, 16000, 16001, 16319]
    pool = oracle.synth(88, 0, len(lens), 16319)
    clips = [pool[k][:L] for k, L in enumerate(lens)]
    assert [m.window_frame_count(L) for L in lens] == [oracle.num_frames(L, om.cfg) for L in lens]
    buf, offs, ln = _pack(clips)
    out = _run(m, _device(buf), offs, ln)
    _check_rows(m, out, [_compose(oracle, om, c) for c in clips], what="fft512")
    m.close()
