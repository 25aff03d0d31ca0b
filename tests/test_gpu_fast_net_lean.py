"""-m gpu: the fast kernel's network half after it shed vector work that changes no bit (profiles/net_lean.md): the rotating-set contraction loop forms
a k-step's operand addresses once for the lo and the hi halves, and the maxima / clamps of the block epilogues, the pools, the in-place split and the
FULLY_CONNECTED clamp are single instructions (csrc/kws_fast_maxmin.h).  Both are identities, so every bar is one that stood before.

Shipped graphs (the headline 49x40 float32 graph, its 49x13 twin, the 49x40 int8 graph whose two-wave form shares the front end), KWS_MODE_FAST:
  * batch sizes 1, 63, 64, 65 and the plan's resident wave count - 1, + 0, + 1: a wave with a single clip, a ragged last trip, a tail pass with and
    without a partner.  A clip's bits do not depend on the batch it arrives in; float32 scores are within fast_tolerance()'s 1e-4 of the oracle's, the
    int8 graph (exact from its input tensor on) has at most 2 % of the bench clips with a changed score (test_gpu_fast_mode.py's bar).
  * 256 hard clips -- 64 each of word_silence (digitally silent frames), bursts, quiet_noise and near_constant (tests/kws_families.py): float32 within
    1e-4 of the oracle, every clip that ended in the exact kernels (found by classifying each clip alone) carries KWS_MODE_EXACT's bits, kws_fast_fallback_count / kws_fast_exact_count
    are the PARENT's (PARENT_COUNTS: taken by running hard_counts() below on the library built from the commit before this change, same clips), and a
    handle's second and third call give the first call's bits.

Synthetic float32 graphs, one per contraction form behind the changed code, on the development build (KWS_DEV_FAST_ENTRY=1: every call starts in the first
tier; KWS_DEV_FAST_WPS=3: the three-wave build): row tiles 4 / 2 / 1, channel tiles 1 / 2, fragments from L2 (KWS_DEV_FAST_B_GLOBAL=1: the
rotating-set loop for every tile shape, and fast_conv_small_h for a last block of three k-steps) and from LDS (the two-set loop, the shared epilogues; which
blocks the plan keeps there is asserted through kws_fast_lds_fragments), pooled on the accumulators (pool >= 4) and from the staging image (pool 2).  The
rotating-set loop on fragments in LDS (the 40-filter instantiations' 4 x 2 tiles) is compiled in but no plan reaches it: SYNTH["f40_c13_42"] has the arithmetic.  First blocks of 5 and 7 taps: image rows -3 .. -1 and 49 .. 51 are
asked for by every clip and must read zeros.  128 bench clips each, 1e-4 against the oracle; some clips must stay in the first tier."""
import multiprocessing as mp
import os

import numpy as np
import pytest

from kws_families import family, word_waveforms
from kws_testlib import MODELS, ROOT, Oracle, OracleModel, bits, synth_model_blob

pytestmark = pytest.mark.gpu

FAST_SCORE_TOL = 1e-4
MODEL_NAMES = ("cfg2_mfcc40_f32.kwsm", "l476_no_yes_f32.kwsm", "cfg2_mfcc40_int8.kwsm")
FAMILY_NAMES = ("word_silence", "bursts", "quiet_noise", "near_constant")
N_FAMILY = 64
N_SYNTH = 128
# (kws_fast_fallback_count, kws_fast_exact_count) of the parent commit's library on hard_set(): see the module docstring
PARENT_COUNTS = {
    "cfg2_mfcc40_f32.kwsm": (67, 65),
    "l476_no_yes_f32.kwsm": (45, 37),
    "cfg2_mfcc40_int8.kwsm": (69, 68),
}

# (out channels, taps, pool) per block: 49 rows -> 4 row tiles; pool 2 -> 25 rows -> 2; then <= 13 rows -> 1.  (A negative pool is VALID pooling: the plan takes
# a SAME pool only where it pads nothing, which 4 over 49 or 25 rows would.)
F40 = dict(num_filters=40, ncep=40, low=300, high=0)
SYNTH = {
    # <4, 2> (5 taps), <2, 1>, <1, 2>; pooled from the staging image twice
    "l2_42_21_12": (dict(F40, seed=81, blocks=((30, 5, 2), (12, 3, 2), (20, 3, 7)), n_labels=4), True, 0b000),
    # <4, 1> (5 taps), <2, 2> pooled on the accumulators, then a block of 3 k-steps: fast_conv_small_h
    # (logit_std: a calibrated head -- with the generator's plain one this graph's softmax is saturated and every score error vanishes)
    "l2_41_22_small": (dict(F40, seed=82, blocks=((16, 5, 2), (24, 3, -4), (8, 3, 6)), n_labels=3, logit_std=3.5), True, 0b000),
    # <4, 2> with 7 taps (rows -3 .. 51, 9 k-steps: whole trips of three) pooled on the accumulators, then <1, 1> with 9 k-steps (past fast_conv_small_h's eight)
    "l2_42_7taps_11": (dict(F40, seed=83, blocks=((32, 7, -4), (8, 9, 6)), n_labels=5), True, 0b00),
    # no development switch for the fragments, 13 cepstra behind 32 filters (the twin's front end, twelve waves): the plan gives the LDS block's spare room
    # to ONE block's fragments -- the <2, 1> block here (the 4 x 2 block's 12 KB do not fit: L2), the <4, 1> block of 7 taps in the next graph: the two-set loop
    "lds_42_21_12": (dict(seed=84, ncep=13, blocks=((30, 5, 2), (12, 3, 2), (20, 3, 7)), n_labels=4), False, 0b010),
    "lds_41_22_11": (dict(seed=85, ncep=13, blocks=((16, 7, 2), (24, 3, -4), (8, 3, 6)), n_labels=3), False, 0b001),
    # The 40-filter front end with 13 cepstra and NO development switch for the fragments: a 4 x 2 first block of 3 k-steps (12 KB of fragments).  This is the
    # graph that WOULD run the rotating-set loop on fragments in LDS (fast_conv_tiles_h<4, 2, false, true>) if a plan could keep them there.  None can: four row
    # tiles mean >= 49 image rows of 44 floats, 13 632 B per wave, and the plan keeps fragments in LDS only while twelve waves fit beside them -- 12 x 13 632 =
    # 163 584 of 163 840 B, 256 B for tables and fragments together.  The expected mask says so: the day a plan change makes that instantiation reachable, this
    # graph fails here and gets its oracle comparison on the LDS form.
    "f40_c13_42": (dict(F40, ncep=13, seed=86, blocks=((30, 5, 2), (12, 3, 2), (20, 3, 7)), n_labels=4), False, 0b000),
}


@pytest.fixture(scope="module")
def pkg():
    import sys
    sys.path.insert(0, ROOT)
    import torch  # noqa: F401
    from __graft_entry__ import load_package
    return load_package()


_W = {}


def _oracle_worker(args):
    path, pcm = args
    if path not in _W:
        _W[path] = OracleModel(_W.setdefault("oracle", Oracle()), path)
    return _W[path].run_batch(pcm)


@pytest.fixture(scope="module")
def pool():
    with mp.get_context("spawn").Pool(min(16, len(os.sched_getaffinity(0)))) as p:
        yield p


def oracle_scores(pool, path, pcm, chunk=128):
    return np.concatenate(pool.map(_oracle_worker, [(path, pcm[i:i + chunk]) for i in range(0, len(pcm), chunk)]))


def hard_set(pkg):
    """host int16 [256][16000]: 64 clips each of FAMILY_NAMES (word_silence made on the GPU by kws_mix_audio_device, as dataset-curation.py pads a short word)"""
    import torch
    fam = {}
    for i, name in enumerate(FAMILY_NAMES):
        if name != "word_silence":
            fam[name] = family(name, N_FAMILY, seed=60 + i)
            continue
        w, ln = word_waveforms(N_FAMILY, 60 + i)
        words, lens = torch.from_numpy(w).to("cuda:0"), torch.from_numpy(ln).to("cuda:0")
        out = torch.zeros((N_FAMILY, 16000), dtype=torch.int16, device="cuda:0")
        pkg.mix_audio_device(words.data_ptr(), lens.data_ptr(), 16000, None, 0, None, 1.0, 0.0, N_FAMILY, 16000, out.data_ptr())
        torch.cuda.synchronize()
        fam[name] = out.cpu().numpy()
    return np.ascontiguousarray(np.concatenate([fam[n] for n in FAMILY_NAMES]))


def run(pkg, gm, pcm_t, mode=None):
    import torch
    n = pcm_t.shape[0]
    gm.set_mode(pkg.MODE_FAST if mode is None else mode)
    s = torch.full((n, gm.n_labels), float("nan"), dtype=torch.float32, device="cuda:0")
    gm.run_classifier_batch_device(pcm_t.data_ptr(), n, s.data_ptr(), None, None)
    torch.cuda.synchronize()
    return s.cpu().numpy()


def hard_counts(pkg, name, hard=None):
    """(handed on, ended in the exact kernels) of one fast call on the hard set, and its scores"""
    import torch
    hard = hard_set(pkg) if hard is None else hard
    gm = pkg.Model(os.path.join(MODELS, name), device=0)
    s = run(pkg, gm, torch.from_numpy(hard).to("cuda:0"))
    counts = (gm.fast_fallback_count(), gm.fast_exact_count())
    gm.close()
    return counts, s


@pytest.fixture(scope="module")
def hard(pkg):
    return hard_set(pkg)


@pytest.mark.parametrize("name", MODEL_NAMES)
def test_batch_sizes_around_a_wave_and_around_the_grid(name, pkg, pool):
    import torch
    path = os.path.join(MODELS, name)
    gm = pkg.Model(path, device=0)
    tol = gm.fast_tolerance()
    is_float = bool(gm.is_float)
    assert tol["entry_tier"] == 1 and (not is_float or tol["fused_waves_per_simd"] == 3), tol
    waves = 256 * (tol["fused_waves"] if is_float else 8)
    host = Oracle().synth(0, 0, waves + 1)
    so = oracle_scores(pool, path, host)
    dev = torch.from_numpy(host).to("cuda:0")
    whole = run(pkg, gm, dev)
    d = np.abs(whole - so)
    print("\n%s: %d waves; %d bench clips: max |score - oracle| = %.3g, %d handed on" % (name, waves, waves + 1, d.max(), gm.fast_fallback_count()))
    assert not np.isnan(whole).any()
    if is_float:
        assert d.max() <= FAST_SCORE_TOL
        assert gm.fast_fallback_count() == 0
    else:
        assert (d.max(axis=1) > 0).mean() <= 0.02
    for n in (1, 63, 64, 65, waves - 1, waves):
        got = run(pkg, gm, dev[:n].contiguous())
        assert (bits(got) == bits(whole[:n])).all(), "%s: %d clips: %d scores differ from the same clips' in a batch of %d" % (name, n, int((bits(got) != bits(whole[:n])).sum()), waves + 1)
    gm.close()


@pytest.mark.parametrize("name", MODEL_NAMES)
def test_hard_clips_keep_the_bar_the_exact_bits_and_the_parents_counts(name, pkg, pool, hard):
    import torch
    path = os.path.join(MODELS, name)
    so = oracle_scores(pool, path, hard)
    gm = pkg.Model(path, device=0)
    is_float = bool(gm.is_float)
    dev = torch.from_numpy(hard).to("cuda:0")
    s = run(pkg, gm, dev)
    counts = (gm.fast_fallback_count(), gm.fast_exact_count())
    second, third = run(pkg, gm, dev), run(pkg, gm, dev)
    se = run(pkg, gm, dev, mode=pkg.MODE_EXACT)
    same = (bits(s) == bits(se)).all(axis=1)
    per = {n: float(np.abs(s - so)[i * N_FAMILY:(i + 1) * N_FAMILY].max()) for i, n in enumerate(FAMILY_NAMES)}
    print("\n%s: families %s; handed on %d, ended in the exact kernels %d (parent: %s), %d clips carry the exact mode's bits" % (name, per, counts[0], counts[1], PARENT_COUNTS[name], int(same.sum())))
    assert not np.isnan(s).any()
    if is_float:
        assert max(per.values()) <= FAST_SCORE_TOL
        assert np.abs(se - so).max() <= 1e-6
    else:
        assert (bits(se) == bits(so)).all()
    # The library reports how MANY clips each tier handed on, not which.  A clip's route and bits do not depend on the batch it arrives in (the test above), so
    # every clip is classified once more ALONE: its call's two counts say whether it was handed on and whether it ended in the exact kernels, its bits
    # must be the batch's, and a clip that ended in the exact kernels must carry KWS_MODE_EXACT's bits -- clip by clip, not by count.
    assert counts[1] <= counts[0] and int(same.sum()) >= counts[1]
    on, ended = np.zeros(len(hard), bool), np.zeros(len(hard), bool)
    for i in range(len(hard)):
        one = run(pkg, gm, dev[i:i + 1])
        on[i], ended[i] = gm.fast_fallback_count() == 1, gm.fast_exact_count() == 1
        assert (bits(one[0]) == bits(s[i])).all(), "%s: clip %d alone differs from the same clip in the batch" % (name, i)
    assert (int(on.sum()), int(ended.sum())) == counts, ((int(on.sum()), int(ended.sum())), counts)
    assert same[ended].all(), "%s: clips %s ended in the exact kernels without the exact mode's bits" % (name, np.nonzero(ended & ~same)[0].tolist())
    if is_float:
        assert np.abs(s - se)[~ended].max(initial=0.0) <= FAST_SCORE_TOL
    assert counts == PARENT_COUNTS[name]
    assert (bits(second) == bits(s)).all() and (bits(third) == bits(s)).all()
    gm.close()


@pytest.mark.parametrize("graph", sorted(SYNTH))
def test_every_contraction_form_against_the_oracle(graph, dev_pkg, pool, tmp_path, monkeypatch):
    import sys
    import torch
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from dequantize_model import dequantize
    kw, from_l2, lds_mask = SYNTH[graph]
    path = str(tmp_path / (graph + ".kwsm"))
    with open(path, "wb") as f:
        f.write(dequantize(synth_model_blob(**kw)))
    monkeypatch.setenv("KWS_DEV_FAST_ENTRY", "1")
    monkeypatch.setenv("KWS_DEV_FAST_WPS", "3")
    if from_l2:
        monkeypatch.setenv("KWS_DEV_FAST_B_GLOBAL", "1")
    else:
        monkeypatch.delenv("KWS_DEV_FAST_B_GLOBAL", raising=False)
    gm = dev_pkg.Model(path, device=0)
    tol = gm.fast_tolerance()
    assert gm.fast_is_fused and tol["fused_waves_per_simd"] == 3, tol
    # which blocks' fragments the plan kept in LDS (kws_fast_lds_fragments): what decides between the rotating-set and the two-set loop
    assert gm.fast_lds_fragments() == lds_mask, "%s: fragments in LDS for blocks %s, expected %s" % (graph, bin(gm.fast_lds_fragments()), bin(lds_mask))
    host = Oracle().synth(0, 0, N_SYNTH)
    so = oracle_scores(pool, path, host)
    dev = torch.from_numpy(host).to("cuda:0")
    got = run(dev_pkg, gm, dev)
    n_fb = gm.fast_fallback_count()
    d = float(np.abs(got - so).max())
    print("\n%s: %d waves per workgroup; %d bench clips: max |score - oracle| = %.3g, %d handed on" % (graph, tol["fused_waves"], N_SYNTH, d, n_fb))
    assert not np.isnan(got).any() and d <= FAST_SCORE_TOL
    assert n_fb < N_SYNTH                                  # the first tier kept clips: the form under test computed scores that are looked at
    assert (bits(run(dev_pkg, gm, dev)) == bits(got)).all()
    gm.close()
