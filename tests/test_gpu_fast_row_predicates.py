"""-m gpu: the three-waves-per-SIMD fast kernel takes the row test of its DCT stores and of cmvnw's sums, stores and guard per value only where a lane can fail
it (csrc/kws_fast.hip: the DCT epilogue's row tiles 0 - 2 with 48 frames or more; fast_cmvn<13, 16, true, true, 9> with 3 x 13 + 9 frames or more), and forms
what is constant per lane -- store base and row stride, the guard's on/off -- once per column block.  Both copies of either phase are compiled into the one
kernel and picked by the frame count, so the cases are the smallest shapes where a row mask, a store base or a zeroed guard coefficient can be wrong:

  * the headline front end (40 filters, 40 cepstra: column blocks of 16 + 16 + 8) in front of a small two-block network at 39, 40, 41, 48, 49 and 50
    frames: cmvnw's last row group (rows 39 .. 51) with no live row, 1, 2, 9, 10 and 11 live rows; the DCT's row tile 3 (rows 48 .. 63) empty, with one
    live row and two; 39 - 41 on the general copies, 48 and up on the lean ones.  (51 and 52 frames: the fused plan refuses the 40-filter front end
    there, whatever the cepstra -- checked on the host build of the library -- so the full last group is the 32-filter graph's, below.)
  * the same front end with 13 and 20 cepstra: one column block with three k-padding columns (zero halves), and a second block of four columns whose
    other twelve lanes have no place in the row (the sink, stride 0, coefficients 0);
  * a 32-filter graph at 49 and at 52 frames: the kernel's other instantiation (four DCT k-groups); 52: every row of the last group and four of tile 3 live.

Per case: 96 clips of the bench's generator plus 8 word_silence clips (kws_families: a word, then digital silence -- silent rows, the pivot on a silent
frame) cut or zero-padded to the case's clip length; scores within 1e-4 of the oracle's (BASELINE's north star, as in test_gpu_fast_mode.py and
test_gpu_fast_cmvn_store.py); batch sizes 1 and the plan's wave count + 1 (the clips repeated: some wave takes a second clip by ticket and meets the stale
halves of its first), every call repeated with identical bits, a clip's bits independent of its batch.  The plan must be laid out for three waves per
SIMD, or the test would pass on another kernel.

The synthetic graphs' gains leave the first tier no room: the product library routes them past it.  As in test_gpu_fast_cmvn_store.py they run on the
development build with KWS_DEV_FAST_ENTRY=1 (every call starts in the first tier; its guard still decides which clips it keeps) and KWS_DEV_FAST_WPS=3,
and some clips must stay in the first tier -- otherwise the code under test would have computed no score that is looked at.  The shipped headline graph
(49 frames, no switch) is held by test_gpu_fast_cmvn_store.py and test_gpu_fast_net_lean.py.

The feature-emitting forms (kws_fast_kernel<..., NET = false>) exist in the two-waves-per-SIMD build only, whose code this change leaves as it was: their
features against the oracle stay with test_gpu_fast_mode.py."""
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


CASES = {"f40_c40_%d_frames" % n: (dict(F40, seed=300 + n, ncep=40, raw_samples=samples(n)), n) for n in (39, 40, 41, 48, 49, 50)}
CASES["f40_c13_49_frames"] = (dict(F40, seed=401, ncep=13), 49)
CASES["f40_c20_49_frames"] = (dict(F40, seed=402, ncep=20), 49)
CASES["f32_c13_49_frames"] = (dict(NET, seed=403, num_filters=32, ncep=13), 49)
CASES["f32_c13_52_frames"] = (dict(NET, seed=404, num_filters=32, ncep=13, raw_samples=samples(52)), 52)


def case_blob(name):
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from dequantize_model import dequantize
    return dequantize(synth_model_blob(**CASES[name][0]))


def case_clips(name):
    """host int16 [N_SYNTH + N_SILENCE][clip length]"""
    n = CASES[name][0].get("raw_samples", 16000)
    words = family("word_silence", N_SILENCE, seed=70)
    quiet = np.zeros((N_SILENCE, n), dtype=np.int16)
    quiet[:, :min(n, words.shape[1])] = words[:, :n]
    return np.ascontiguousarray(np.concatenate([Oracle().synth(7, 0, N_SYNTH, n), quiet]))


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
    import torch
    n = pcm_t.shape[0]
    gm.set_mode(pkg.MODE_FAST)
    s = torch.full((n, gm.n_labels), float("nan"), dtype=torch.float32, device="cuda:0")
    gm.run_classifier_batch_device(pcm_t.data_ptr(), n, s.data_ptr(), None, None)
    torch.cuda.synchronize()
    return s.cpu().numpy()


@pytest.mark.parametrize("name", sorted(CASES))
def test_row_predicates_at_every_fill_of_the_last_row_group(name, dev_pkg, pool, tmp_path, monkeypatch):
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

    whole = run(pkg, gm, dev)
    n_fb = gm.fast_fallback_count()
    d = np.abs(whole - so[idx])
    print("\n%s: %d frames, %d waves per workgroup; %d clips: max |score - oracle| = %.3g (silence clips %.3g), %d handed on"
          % (name, gm.n_frames, tol["fused_waves"], waves + 1, d.max(), d[idx >= N_SYNTH].max(), n_fb))
    assert not np.isnan(whole).any() and d.max() <= FAST_SCORE_TOL
    assert n_fb < waves + 1                                  # the first tier kept clips: the code under test computed scores that are looked at
    assert (bits(run(pkg, gm, dev)) == bits(whole)).all()
    # a clip's bits depend neither on its batch nor on which wave took it, first or by ticket
    assert (bits(whole) == bits(whole[:n][idx])).all()
    for i in (0, n - 1):
        one = run(pkg, gm, dev[i:i + 1].contiguous())
        assert (bits(one[0]) == bits(whole[i])).all(), (name, i)
        assert (bits(run(pkg, gm, dev[i:i + 1].contiguous())) == bits(one)).all()
    gm.close()
