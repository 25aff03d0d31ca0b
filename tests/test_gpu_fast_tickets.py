"""-m gpu: how the three-waves-per-SIMD fast kernel (csrc/kws_fast.hip) deals its clips out: tickets come from eight heads (csrc/kws_fast_ticket.h;
tests/test_fast_ticket_host.py deals the same mapping out on the CPU).  A workgroup draws from the head of its block index modulo 8; a wave whose head is past
the last clip finishes its clip without a successor (no paired tail pass), then walks the other heads; the last wave out zeroes all of them.

What can go wrong: a clip nobody takes (its scores keep the NaN they were filled with) or two waves take (not visible in the scores -- the host test's
part), a head that is not zero when the next launch starts (that launch skips clips), a clip that follows a walk and meets a stash or a wrap sample that is
not its own (scores move).  So, for the 49x40 graph (W = 11 waves per workgroup) and its 49x13 twin (W = 12):

  * batch sizes 1, W - 1, W, W + 1, 8 W +- 1 (fewer clips than waves: every head is exhausted from the first draw), 256 W - 1, 256 W (the full grid, no ticket
    is a clip), 256 W + k for k = 1 .. 9 (tickets on some heads only: every wave of the other heads walks), 2 x 256 W + 3 and 4 099; the scores buffer holds NaN
    before each call and none after it; every batch's bits are the prefix of the largest batch's; the first 1 024 clips are within 1e-4 of the oracle's;
  * six calls back to back, large and small in turn, give those bits again: the heads come back clean.

And frame counts 39 .. 52 with the synthetic graphs of tests/test_gpu_fast_full_pass.py (its front ends and network; 51 and 52 frames behind 32 filters, the
fused plan refuses them behind 40), 2 x the grid's waves + 3 clips so that every wave has a successor by ticket and the last three come from three heads
only: at 8 k + 1 frames the successor's last frame rides in the clip's tail pass, at the others a pass's requests one and two passes ahead meet their clamp
on a clip that a ticket brought.  Within 1e-4 of the oracle, launches bit-identical, a clip's bits independent of its batch and of the wave that took it.
(The touches of a clip's last passes were to warm the successor's first frames, and its wrap sample to be requested a clip ahead: built, measured slower,
not in the tree -- profiles/clip_edges.md; these cases are what that form was held to.)  As there, they run on the development build with
KWS_DEV_FAST_ENTRY=1 and KWS_DEV_FAST_WPS=3, and some clips must stay in the first tier."""
import multiprocessing as mp
import os

import numpy as np
import pytest

from kws_families import family
from kws_testlib import MODELS, ROOT, Oracle, OracleModel, bits, synth_model_blob

pytestmark = pytest.mark.gpu

FAST_SCORE_TOL = 1e-4          # north_star: "per-class scores match the reference C path within 1e-4 fp32"
N_ORACLE = 1024
GRAPHS = {"cfg2_mfcc40_f32.kwsm": 11, "l476_no_yes_f32.kwsm": 12}

NET = dict(blocks=((16, 3, -2), (8, 3, -2)), n_labels=3, logit_std=3.5)      # test_gpu_fast_full_pass.py's network and front ends
F40 = dict(NET, num_filters=40, low=300, high=0)
F32 = dict(NET, num_filters=32, ncep=13)
N_SYNTH, N_SILENCE = 96, 8


def samples(n_frames):
    return 320 * (n_frames + 1)                  # 20 ms frames and stride at 16 kHz: frames = floor((n - 320) / 320)


FRAME_CASES = {"f40_c40_%d_frames" % n: (dict(F40, seed=500 + n, ncep=40, raw_samples=samples(n)), n) for n in range(39, 51)}
FRAME_CASES.update({"f32_c13_%d_frames" % n: (dict(F32, seed=553 + n, raw_samples=samples(n)), n) for n in (51, 52)})


def batch_sizes(w):
    return [1, w - 1, w, w + 1, 8 * w - 1, 8 * w + 1, 256 * w - 1, 256 * w] + [256 * w + k for k in range(1, 10)] + [2 * 256 * w + 3, 4099]


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


@pytest.fixture(scope="module")
def bench_clips(pkg):
    """the bench's generator: (device int16 [largest batch][16000], host copy of the first N_ORACLE clips)"""
    import torch
    n = max(max(batch_sizes(w)) for w in GRAPHS.values())
    dev = torch.empty((n, 16000), dtype=torch.int16, device="cuda:0")
    pkg.synth_clips_device(0, 0, n, 16000, dev.data_ptr())
    torch.cuda.synchronize()
    return dev, dev[:N_ORACLE].cpu().numpy()


def run(pkg, gm, pcm_t):
    """(scores, clips handed on); the scores buffer holds NaN when the call starts"""
    import torch
    n = pcm_t.shape[0]
    gm.set_mode(pkg.MODE_FAST)
    s = torch.full((n, gm.n_labels), float("nan"), dtype=torch.float32, device="cuda:0")
    gm.run_classifier_batch_device(pcm_t.data_ptr(), n, s.data_ptr(), None, None)
    torch.cuda.synchronize()
    return s.cpu().numpy(), gm.fast_fallback_count()


@pytest.mark.parametrize("graph", sorted(GRAPHS))
def test_every_batch_size_takes_every_clip_once_and_leaves_the_heads_clean(graph, pkg, pool, bench_clips):
    path = os.path.join(MODELS, graph)
    gm = pkg.Model(path, device=0)
    tol = gm.fast_tolerance()
    w = GRAPHS[graph]
    # the path under test: the plan is laid out for three waves per SIMD, W waves per workgroup, and every batch call starts in the fast kernel
    assert gm.fast_is_fused and tol["fused_waves_per_simd"] == 3 and tol["fused_waves"] == w and tol["entry_tier"] == 1, tol
    dev, host = bench_clips
    so = np.concatenate(pool.map(_oracle_worker, [(path, host[i:i + 64]) for i in range(0, N_ORACLE, 64)]))
    sizes = batch_sizes(w)
    largest = max(sizes)
    whole, n_fb = run(pkg, gm, dev[:largest])
    d = float(np.abs(whole[:N_ORACLE] - so).max())
    print("\n%s: %d waves per workgroup; %d clips: max |score - oracle| over the first %d = %.3g, %d handed on" % (graph, w, largest, N_ORACLE, d, n_fb))
    assert not np.isnan(whole).any()
    assert d <= FAST_SCORE_TOL
    for n in sizes:
        got, _ = run(pkg, gm, dev[:n])
        assert not np.isnan(got).any(), (graph, n, np.flatnonzero(np.isnan(got).any(axis=1))[:8])
        assert (bits(got) == bits(whole[:n])).all(), (graph, n)
    # the heads come back clean: large and small in turn, nothing in between
    for n in (largest, 1, 256 * w + 5, w + 1, largest, 8 * w - 1):
        got, _ = run(pkg, gm, dev[:n])
        assert not np.isnan(got).any() and (bits(got) == bits(whole[:n])).all(), (graph, n)
    gm.close()


def frame_case_blob(name):
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from dequantize_model import dequantize
    return dequantize(synth_model_blob(**FRAME_CASES[name][0]))


def frame_case_clips(name):
    """host int16 [N_SYNTH + N_SILENCE][clip length]: the bench's generator, and words followed by digital silence"""
    n = FRAME_CASES[name][0]["raw_samples"]
    words = family("word_silence", N_SILENCE, seed=71)
    quiet = np.zeros((N_SILENCE, n), dtype=np.int16)
    quiet[:, :min(n, words.shape[1])] = words[:, :n]
    return np.ascontiguousarray(np.concatenate([Oracle().synth(11, 0, N_SYNTH, n), quiet]))


@pytest.mark.parametrize("name", sorted(FRAME_CASES))
def test_clips_by_ticket_at_every_frame_count(name, dev_pkg, pool, tmp_path, monkeypatch):
    import torch
    pkg = dev_pkg
    path = str(tmp_path / (name + ".kwsm"))
    with open(path, "wb") as f:
        f.write(frame_case_blob(name))
    monkeypatch.setenv("KWS_DEV_FAST_ENTRY", "1")
    monkeypatch.setenv("KWS_DEV_FAST_WPS", "3")
    gm = pkg.Model(path, device=0)
    tol = gm.fast_tolerance()
    assert gm.n_frames == FRAME_CASES[name][1]
    assert gm.fast_is_fused and tol["fused_waves_per_simd"] == 3, tol
    host = frame_case_clips(name)
    n = len(host)
    so = np.concatenate(pool.map(_oracle_worker, [(path, host[i:i + 26]) for i in range(0, n, 26)]))
    waves = 256 * tol["fused_waves"]
    idx = np.arange(2 * waves + 3) % n                       # every wave takes a second clip, three a third
    dev = torch.from_numpy(np.ascontiguousarray(host[idx])).to("cuda:0")

    whole, n_fb = run(pkg, gm, dev)
    d = np.abs(whole - so[idx])
    print("\n%s: %d frames, %d waves per workgroup; %d clips: max |score - oracle| = %.3g, %d handed on" % (name, gm.n_frames, tol["fused_waves"], len(idx), d.max(), n_fb))
    assert not np.isnan(whole).any() and d.max() <= FAST_SCORE_TOL
    assert n_fb < len(idx)                                   # the first tier kept clips: the code under test computed scores that are looked at
    again, n_fb2 = run(pkg, gm, dev)
    assert (bits(again) == bits(whole)).all() and n_fb2 == n_fb
    # a clip's bits depend neither on its batch nor on which wave took it, first or by ticket, behind whichever clip
    assert (bits(whole) == bits(whole[:n][idx])).all()
    for m in (1, waves + 1):
        part, _ = run(pkg, gm, dev[:m])
        assert not np.isnan(part).any() and (bits(part) == bits(whole[:m])).all(), (name, m)
    gm.close()
