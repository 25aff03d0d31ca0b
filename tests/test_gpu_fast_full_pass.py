"""-m gpu: the spectral pass loop of the three-waves-per-SIMD fast kernel (csrc/kws_fast.hip) -- what it does differently for a pass of eight live frames,
and what it no longer does per pass:

  * the mel phase is compiled twice, and a pass with eight frames left takes the copy without frame predicates (one batch of reads, unpredicated stores);
    a last pass of fewer frames, and the tail pass, keep the general copy;
  * the sample requests are the clip's base (scalar) + a 32-bit byte offset per lane that advances by eight frames per pass, clamped by one minimum
    against the lane's offset in the last frame; only the clip's first request carries the guard against reading in front of the PCM buffer;
  * a pass parks a frame's energy itself, and its zero handling and log are taken once per clip in front of the DCT.

So the cases are the frame counts at which a pass picks the other copy, an offset meets its clamp, or a parked energy arrives by another way:

  * the headline front end (40 filters, 40 cepstra) in front of a small two-block network at 40 and 48 frames (full passes only, no tail), 41 and 49 (a
    tail pass of one frame: paired with the next clip's last frame, whose energy waits in the stash), 42 and 50 (a tail pass of two) -- and at 39, 43 and
    47 frames, whose last pass holds 7, 3 and 7 frames and takes the general copy behind full ones; the requests one and two passes ahead run into the clamp
    at every one of them;
  * a 32-filter graph (the kernel's other instantiation) at 49 frames and at 52 (six full passes and a last one of four).
    (51 and 52 frames behind 40 filters: the fused plan refuses them -- checked on the host build of the library, like every shape here.)

Per case: 96 clips of the bench's generator plus 8 word_silence clips (kws_families: a word, then digital silence -- frames of energy exactly 0, the
zero handling of the deferred log, and the silent-row test that compares column 0 with log(FLT_EPSILON) bit for bit) cut or zero-padded to the case's clip
length; scores within 1e-4 of the oracle's; batch sizes 1 and the plan's wave count + 1 (some wave takes a second clip by ticket), clip 0 of the buffer on
its own (nothing of the allocation lies in front of its first sample), every call twice with identical bits and hand-on counts, a clip's bits
independent of its batch.  The plan must be laid out for three waves per SIMD, or the test would pass on another kernel.

As in test_gpu_fast_row_predicates.py the synthetic graphs run on the development build with KWS_DEV_FAST_ENTRY=1 and KWS_DEV_FAST_WPS=3, and some clips
must stay in the first tier."""
import multiprocessing as mp
import os

import numpy as np
import pytest

from kws_families import family
from kws_testlib import ROOT, Oracle, OracleModel, bits, synth_model_blob

pytestmark = pytest.mark.gpu

FAST_SCORE_TOL = 1e-4          # north_star: "per-class scores match the reference C path within 1e-4 fp32"
N_SYNTH = 96
N_SILENCE = 8

NET = dict(blocks=((16, 3, -2), (8, 3, -2)), n_labels=3, logit_std=3.5)      # VALID pools: any row count; a calibrated head: the softmax is not saturated
F40 = dict(NET, num_filters=40, low=300, high=0)


def samples(n_frames):
    return 320 * (n_frames + 1)                  # 20 ms frames and stride at 16 kHz: frames = floor((n - 320) / 320)


FULL = (40, 41, 42, 48, 49, 50)                  # every eight-frame pass full; 41 / 49 and 42 / 50 with a tail pass
GENERAL = (39, 43, 47)                           # the last pass holds 7, 3, 7 frames
CASES = {"f40_c40_%d_frames" % n: (dict(F40, seed=500 + n, ncep=40, raw_samples=samples(n)), n) for n in FULL + GENERAL}
CASES["f32_c13_49_frames"] = (dict(NET, seed=603, num_filters=32, ncep=13), 49)
CASES["f32_c13_52_frames"] = (dict(NET, seed=604, num_filters=32, ncep=13, raw_samples=samples(52)), 52)


def case_blob(name):
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from dequantize_model import dequantize
    return dequantize(synth_model_blob(**CASES[name][0]))


def case_clips(name):
    """host int16 [N_SYNTH + N_SILENCE][clip length]"""
    n = CASES[name][0].get("raw_samples", 16000)
    words = family("word_silence", N_SILENCE, seed=71)
    quiet = np.zeros((N_SILENCE, n), dtype=np.int16)
    quiet[:, :min(n, words.shape[1])] = words[:, :n]
    return np.ascontiguousarray(np.concatenate([Oracle().synth(11, 0, N_SYNTH, n), quiet]))


_W = {}


def _oracle_worker(args):
    path, pcm = args
    if path not in _W:
        _W[path] = OracleModel(_W.setdefault("oracle", Oracle()), path)
    return _W[path].run_batch(pcm)


@pytest.fixture(scope="module")
def pool():
    with mp.get_context("spawn").Pool(min(8, len(os.sched_getaffinity(0)))) as p:
        yield p


def run(pkg, gm, pcm_t):
    """(scores, clips handed on)"""
    import torch
    n = pcm_t.shape[0]
    gm.set_mode(pkg.MODE_FAST)
    s = torch.full((n, gm.n_labels), float("nan"), dtype=torch.float32, device="cuda:0")
    gm.run_classifier_batch_device(pcm_t.data_ptr(), n, s.data_ptr(), None, None)
    torch.cuda.synchronize()
    return s.cpu().numpy(), gm.fast_fallback_count()


@pytest.mark.parametrize("name", sorted(CASES))
def test_pass_loop_at_every_fill_of_the_last_pass(name, dev_pkg, pool, tmp_path, monkeypatch):
    import torch
    pkg = dev_pkg
    path = str(tmp_path / (name + ".kwsm"))
    with open(path, "wb") as f:
        f.write(case_blob(name))
    monkeypatch.setenv("KWS_DEV_FAST_ENTRY", "1")
    monkeypatch.setenv("KWS_DEV_FAST_WPS", "3")
    gm = pkg.Model(path, device=0)
    tol = gm.fast_tolerance()
    assert gm.n_frames == CASES[name][1]
    assert gm.fast_is_fused and tol["fused_waves_per_simd"] == 3, tol
    host = case_clips(name)
    n = len(host)
    so = np.concatenate(pool.map(_oracle_worker, [(path, host[i:i + 26]) for i in range(0, n, 26)]))
    waves = 256 * tol["fused_waves"]
    idx = np.arange(waves + 1) % n
    dev = torch.from_numpy(np.ascontiguousarray(host[idx])).to("cuda:0")

    whole, n_fb = run(pkg, gm, dev)
    d = np.abs(whole - so[idx])
    print("\n%s: %d frames, %d waves per workgroup; %d clips: max |score - oracle| = %.3g (silence clips %.3g), %d handed on"
          % (name, gm.n_frames, tol["fused_waves"], waves + 1, d.max(), d[idx >= N_SYNTH].max(), n_fb))
    assert not np.isnan(whole).any() and d.max() <= FAST_SCORE_TOL
    assert n_fb < waves + 1                                  # the first tier kept clips: the code under test computed scores that are looked at
    again, n_fb2 = run(pkg, gm, dev)
    assert (bits(again) == bits(whole)).all() and n_fb2 == n_fb
    # a clip's bits depend neither on its batch nor on which wave took it, first or by ticket
    assert (bits(whole) == bits(whole[:n][idx])).all()
    for i in (0, n - 1):                                     # clip 0 of the buffer; a word_silence clip
        one, fb1 = run(pkg, gm, dev[i:i + 1])
        assert (bits(one[0]) == bits(whole[i])).all(), (name, i)
        two, fb2 = run(pkg, gm, dev[i:i + 1])
        assert (bits(two) == bits(one)).all() and fb2 == fb1
    gm.close()
