"""-m gpu: the three-waves-per-SIMD fast kernel's cmvnw stores the first convolution block's operands (csrc/kws_fast.hip: fast_cmvn<..., SPLIT>; KwsFastPlan::presplit):
every feature leaves cmvnw as its two binary16 halves of x 2^10, laid out per 16-column block inside the fp32 row, and the block no longer converts its image.

What can go wrong there, and the smallest shapes that show it:
  * the row layout -- 40 columns (blocks of 16 + 16 + 8, the last block's lo halves in the row's padding), 13 columns (one block, three zero-padded channels),
    and first blocks of 5 and 7 k-steps whose operand table walks the groups in the new order;
  * B = 1 (no paired tail pass) and B = 2 880 (a few waves take a second clip by ticket: stale halves in a wave's image and padding meet a new clip);
  * the clip-independent scale at the inputs where cmvnw's reciprocal deviation is largest: 256 clips each of word_silence, bursts, quiet_noise and near_constant
    (tests/kws_families.py: column 0's replayed means, silent-frame pivots, near-zero variances).
Bar: every score within 1e-4 of the oracle's (BASELINE's north star, as in test_gpu_fast_mode.py), repeated launches bit-identical, no clip of the bench's
synthetic input handed on by the shipped graphs, and on the families every clip that ended in the exact kernels carries the exact mode's bits.

The two synthetic graphs' gains leave the first tier no room: the product library routes them past it (entry tier 2) and lays them out for two waves per SIMD.
They are here for block 0's operand table in cmvnw's layout, so they are built as test_gpu_fast_mode.py's depthwise-separable graphs are: on the development
build of the library (conftest.py: dev_pkg) with KWS_DEV_FAST_ENTRY=1 (every batch call starts in the first tier; its guard still decides which clips it
keeps) and KWS_DEV_FAST_WPS=3.  Their guards hand on what they hand on (the count is printed, not bounded: the parent promises 0 for the shipped graphs only),
but some bench clips must stay in the first tier -- otherwise the table under test would have computed no score that is looked at."""
import multiprocessing as mp
import os

import numpy as np
import pytest

from kws_families import family, word_waveforms
from kws_testlib import MODELS, ROOT, Oracle, OracleModel, bits, synth_model_blob

pytestmark = pytest.mark.gpu

FAST_SCORE_TOL = 1e-4          # north_star: "per-class scores match the reference C path within 1e-4 fp32"
B_BENCH = 2880                 # the 49x40 graph: 256 workgroups x 11 waves = 2 816 first clips, 64 tickets; the 49x13 twin: 12 waves, 3 072 > B -- every wave one clip
B_TICKETS = 3200               # ... so the twin's second clips come from a batch of its own size class
N_FAMILY = 256
FAMILY_NAMES = ("word_silence", "bursts", "quiet_noise", "near_constant")

# (test_gpu_fast_mode.py: FUSED_POOL_GRAPHS) first blocks whose fragments come from L2 in k-step counts that are not multiples of three
SYNTH = {
    "w3_l2_fragments_7_ksteps": dict(seed=67, num_filters=40, ncep=40, low=300, high=0, blocks=((30, 5, 7), (10, 5, 7)), n_labels=4),    # 5 taps x 5 groups = 25 -> 7 k-steps
    "w3_l2_fragments_5_ksteps": dict(seed=68, num_filters=40, ncep=40, low=300, high=0, blocks=((24, 4, 7), (12, 3, 7)), n_labels=5),    # 4 taps x 5 groups = 20 -> 5 k-steps
}
GRAPHS = ("cfg2_mfcc40_f32.kwsm", "l476_no_yes_f32.kwsm") + tuple(sorted(SYNTH))


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


@pytest.fixture(scope="module")
def clips(pkg):
    """host int16: the bench's synthetic clips (seed 0, from clip 0) and the four families, made once for every graph"""
    import torch
    bench = Oracle().synth(0, 0, B_TICKETS)
    fam = {}
    for i, name in enumerate(FAMILY_NAMES):
        if name != "word_silence":
            fam[name] = family(name, N_FAMILY, seed=40 + i)
            continue
        # word, then digital silence: made on the GPU by kws_mix_audio_device (no background: dataset-curation.py's zero padding)
        w, ln = word_waveforms(N_FAMILY, 40 + i)
        words, lens = torch.from_numpy(w).to("cuda:0"), torch.from_numpy(ln).to("cuda:0")
        out = torch.zeros((N_FAMILY, 16000), dtype=torch.int16, device="cuda:0")
        pkg.mix_audio_device(words.data_ptr(), lens.data_ptr(), 16000, None, 0, None, 1.0, 0.0, N_FAMILY, 16000, out.data_ptr())
        torch.cuda.synchronize()
        fam[name] = out.cpu().numpy()
    return bench, np.ascontiguousarray(np.concatenate([fam[n] for n in FAMILY_NAMES]))


def run_fast(pkg, gm, pcm_t, mode=None):
    import torch
    n = pcm_t.shape[0]
    gm.set_mode(pkg.MODE_FAST if mode is None else mode)
    s = torch.full((n, gm.n_labels), float("nan"), dtype=torch.float32, device="cuda:0")
    gm.run_classifier_batch_device(pcm_t.data_ptr(), n, s.data_ptr(), None, None)
    torch.cuda.synchronize()
    return s.cpu().numpy()


@pytest.mark.parametrize("graph", GRAPHS)
def test_cmvnw_stores_the_first_blocks_operands(graph, pkg, dev_pkg, pool, clips, tmp_path, monkeypatch):
    import sys
    import torch
    synth = graph in SYNTH
    if synth:
        sys.path.insert(0, os.path.join(ROOT, "tools"))
        from dequantize_model import dequantize
        path = str(tmp_path / (graph + ".kwsm"))
        with open(path, "wb") as f:
            f.write(dequantize(synth_model_blob(**SYNTH[graph])))
        pkg = dev_pkg                                # the development switches are read at kws_create, by the development build only
        monkeypatch.setenv("KWS_DEV_FAST_ENTRY", "1")
        monkeypatch.setenv("KWS_DEV_FAST_WPS", "3")
    else:
        path = os.path.join(MODELS, graph)
    gm = pkg.Model(path, device=0)
    tol = gm.fast_tolerance()
    # the path under test: a plan laid out for three waves per SIMD receives block 0's operands from cmvnw (the shipped graphs: test_gpu_fast_mode.py pins 3 x 11 / 12)
    assert gm.fast_is_fused and tol["fused_waves_per_simd"] == 3 and (synth or tol["entry_tier"] == 1), tol
    bench, fam = clips
    more = tol["fused_waves"] * 256 >= B_BENCH                                        # twelve waves per workgroup: 2 880 clips leave every wave of 256 workgroups with one
    so = oracle_scores(pool, path, bench[:B_TICKETS if more else B_BENCH])
    sf = oracle_scores(pool, path, fam)

    # ---- the bench's clips: B = 2 880 (and the next size that outnumbers this plan's waves: some waves take a second clip by ticket), then B = 1
    first = None
    for n_bench in (B_BENCH, B_TICKETS) if more else (B_BENCH,):
        pcm = torch.from_numpy(bench[:n_bench]).to("cuda:0")
        got = run_fast(pkg, gm, pcm)
        n_fb = gm.fast_fallback_count()
        d = float(np.abs(got - so[:n_bench]).max())
        print("\n%s: %d waves per workgroup, sigma_net %.3g; bench clips x %d: max |score - oracle| = %.3g, %d handed on" % (graph, tol["fused_waves"], tol["sigma_net"], n_bench, d, n_fb))
        assert not np.isnan(got).any() and d <= FAST_SCORE_TOL
        if synth:
            assert n_fb < n_bench                                                   # the first tier kept clips: block 0's table computed scores that are checked here
        else:
            assert n_fb == 0
        for rep in range(3):                                                      # which wave takes which clip changes from launch to launch; the bits do not
            assert (bits(run_fast(pkg, gm, pcm)) == bits(got)).all(), (graph, n_bench, rep)
        first = got if first is None else first
        assert (bits(got[:B_BENCH]) == bits(first)).all()
    one = run_fast(pkg, gm, pcm[:1].contiguous())
    assert (bits(one) == bits(first[:1])).all() and np.abs(one - so[:1]).max() <= FAST_SCORE_TOL
    assert (bits(run_fast(pkg, gm, pcm[:1].contiguous())) == bits(one)).all()

    # ---- the families: where cmvnw's reciprocal deviation is largest
    pcm_f = torch.from_numpy(fam).to("cuda:0")
    s = run_fast(pkg, gm, pcm_f)
    n_on, n_exact = gm.fast_fallback_count(), gm.fast_exact_count()
    s_again = run_fast(pkg, gm, pcm_f)
    se = run_fast(pkg, gm, pcm_f, mode=pkg.MODE_EXACT)
    per = {n: float(np.abs(s - sf)[i * N_FAMILY:(i + 1) * N_FAMILY].max()) for i, n in enumerate(FAMILY_NAMES)}
    same = (bits(s) == bits(se)).all(axis=1)
    print("%s: families %s; %d of %d clips handed on, %d ended in the exact kernels, %d carry the exact mode's bits" % (graph, per, n_on, len(fam), n_exact, int(same.sum())))
    assert not np.isnan(s).any() and max(per.values()) <= FAST_SCORE_TOL
    assert (bits(s_again) == bits(s)).all()
    assert np.abs(se - sf).max() <= 1e-6
    # every clip that ended in the exact kernels has their bits (a clip the fast tiers kept differs from them in its last digits).  The library reports how
    # MANY clips each tier handed on, not which: so the count of clips with the exact mode's bits must reach the count that ended there, and a clip WITHOUT
    # those bits -- one a fast tier kept, or one that was handed on and came back wrong -- must still be within the bar of the exact mode's scores
    assert n_exact <= n_on and int(same.sum()) >= n_exact
    assert np.abs(s - se)[~same].max(initial=0.0) <= FAST_SCORE_TOL
    gm.close()

