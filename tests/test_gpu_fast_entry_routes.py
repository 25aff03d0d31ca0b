"""-m gpu: the two routes of a KWS_MODE_FAST batch call that no shipped int8 model takes, forced on the development build with
KWS_DEV_FAST_ENTRY (read at kws_create) for cfg2_mfcc40_int8.kwsm:
  * entry tier 3 -- the exact kernels throughout: scores, features and int8 tensor are KWS_MODE_EXACT's bit for bit and both counts are 0;
  * entry tier 2 of an un-fused graph -- every clip's cepstra from the exact kernels, the fast cmvnw + the int8 network from them, the exact kernels
    for what that hands on: the scores-only call equals the call that also returns features and tensor, every clip handed on was finished by the exact
    kernels, a clip whose features are the exact mode's carries the exact mode's scores, every other clip meets the int8 fast-mode bar
    (test_gpu_fast_mode.py: check_int8_fast_bar) against the exact mode's results on the same handle -- which are the reference's bit for bit.
B = 300 is no multiple of a wave count (some waves take two clips): 268 synthetic clips, then 16 all-zero clips and 16 clips of one constant value each,
whose cmvnw is ill-conditioned -- the second tier must hand them on."""
import os

import numpy as np
import pytest

import test_gpu_fast_mode as fm
from kws_testlib import MODELS, OracleModel, bits

pytestmark = pytest.mark.gpu

NAME = "cfg2_mfcc40_int8.kwsm"
B, N_SYNTH, N_ZERO, SEED = 300, 268, 16, 4300


@pytest.fixture(scope="module")
def clips(dev_pkg):
    import torch
    pcm = torch.zeros((B, 16000), dtype=torch.int16, device="cuda:0")
    dev_pkg.synth_clips_device(SEED, 0, N_SYNTH, 16000, pcm.data_ptr())
    consts = np.random.default_rng(6).integers(-32768, 32767, B - N_SYNTH - N_ZERO)
    pcm[N_SYNTH + N_ZERO:] = torch.from_numpy(consts.astype(np.int16)).to("cuda:0")[:, None]
    torch.cuda.synchronize()
    return pcm


def model(dev_pkg, monkeypatch, entry):
    monkeypatch.setenv("KWS_DEV_FAST_ENTRY", str(entry))
    gm = dev_pkg.Model(os.path.join(MODELS, NAME), device=0)
    assert gm.fast_tolerance()["entry_tier"] == entry
    return gm


def test_entry_tier_3_is_the_exact_mode(dev_pkg, clips, monkeypatch):
    gm = model(dev_pkg, monkeypatch, 3)
    s, f, q = fm.run_device(dev_pkg, gm, dev_pkg.MODE_FAST, clips)
    counts = (gm.fast_fallback_count(), gm.fast_exact_count())
    se, fe, qe = fm.run_device(dev_pkg, gm, dev_pkg.MODE_EXACT, clips)
    assert (bits(s) == bits(se)).all() and (bits(f) == bits(fe)).all() and (q == qe).all()
    assert counts == (0, 0)
    gm.close()


def test_entry_tier_2_from_cepstra_for_an_unfused_graph(dev_pkg, clips, oracle, monkeypatch):
    gm = model(dev_pkg, monkeypatch, 2)
    s, f, q = fm.run_device(dev_pkg, gm, dev_pkg.MODE_FAST, clips)
    n_on, n_exact = gm.fast_fallback_count(), gm.fast_exact_count()
    s_only, _, _ = fm.run_device(dev_pkg, gm, dev_pkg.MODE_FAST, clips, want_f=False)
    n_on_s, n_exact_s = gm.fast_fallback_count(), gm.fast_exact_count()
    se, fe, qe = fm.run_device(dev_pkg, gm, dev_pkg.MODE_EXACT, clips)
    same = (bits(f) == bits(fe)).all(axis=1)
    print("\n%s from exact cepstra, %d clips: %d handed on, %d finished by the exact kernels (scores only: %d, %d); %d clips carry the exact mode's features, "
          "%d of the %d zero / constant clips" % (NAME, B, n_on, n_exact, n_on_s, n_exact_s, int(same.sum()), int(same[N_SYNTH:].sum()), B - N_SYNTH))
    assert (bits(s_only) == bits(s)).all()
    assert n_exact == n_on and n_exact_s == n_on_s
    assert same[N_SYNTH:].all() and n_on >= B - N_SYNTH            # the ill-conditioned clips are handed on and come out exact
    assert (bits(s[same]) == bits(se[same])).all()
    other = ~same
    assert other.any()                                             # ... and the fast cmvnw computed features that are looked at
    fm.check_int8_fast_bar(NAME, OracleModel(oracle, os.path.join(MODELS, NAME)), s[other], f[other], q[other], se[other], fe[other], qe[other])
    gm.close()
