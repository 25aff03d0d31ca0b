"""-m gpu: the general MFCC kernels (csrc/kws_generic.hip) over the whole range of shapes build_dsp_plan admits -- the table of
tests/general_dsp_shapes.py: mixed-radix and degenerate fft lengths, fft 2048 on the cooperative kernel and fft 4096 on the scratch kernel,
2 .. 128 filters, cmvnw windows of 1 / 3 / 301 rows and its global-memory form, odd geometry -- against the oracle, which
tests/test_oracle_vs_reference.py::test_general_envelope_shapes_pinned holds to the compiled reference on the same shapes.  Everything is
KWS_MODE_EXACT and compared bit for bit: no clip masked out, no NaN tolerated (the oracle's features are asserted finite), every word compared.
A shape whose plan names another kernel than the table fails."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import general_dsp_shapes as G
from kws_testlib import MODELS, ROOT, OracleModel, bits

pytestmark = pytest.mark.gpu
N_SYNTH = 66                 # + the four special clips: batches of 70


@pytest.fixture(scope="module")
def pkg():
    sys.path.insert(0, ROOT)
    import torch  # noqa: F401
    from __graft_entry__ import load_package
    return load_package()


@pytest.fixture(scope="module")
def shipped(pkg):
    """the model run_classifier() serves when the float-PCM test is over"""
    return pkg.Model(os.path.join(MODELS, "l476_no_yes.kwsm"))


def differing(a, b):
    return int((bits(a) != bits(b)).sum())


@pytest.mark.parametrize("name", G.NAMES)
def test_every_admitted_shape_bit_exact(name, pkg, oracle, tmp_path):
    import torch
    om = OracleModel(oracle, G.write_model(name, tmp_path))
    gm = pkg.Model(blob=om.blob)
    assert gm.mfcc_kernel == G.SERVED[name][1], (name, gm.mfcc_kernel)
    clips = G.clips(oracle, om.raw_sample_count, N_SYNTH)
    so, fo, qo = om.run_batch(clips, want_features=True)
    assert np.isfinite(fo).all() and np.isfinite(so).all(), name
    for B in (len(clips), 1):                                       # (the batch of one: the last clip, the full-scale alternation)
        s, f, q = gm.run_classifier_batch(clips[-B:], want_features=True)
        assert differing(f, fo[-B:]) == 0, (name, B, differing(f, fo[-B:]), f.size)
        assert (q == qo[-B:]).all() and (bits(s) == bits(so[-B:])).all(), (name, B)
    # the stage API: cepstra before cmvnw (on the last 8 clips: four synthetic, the four special ones), features, then cmvnw + inference
    d = torch.from_numpy(clips).to("cuda:0")
    mf = torch.zeros((len(clips), gm.n_features), dtype=torch.float32, device="cuda:0")
    ft = torch.zeros((len(clips), gm.n_features), dtype=torch.float32, device="cuda:0")
    gm.mfcc_batch_device(d.data_ptr(), len(clips), mf.data_ptr())
    gm.extract_mfcc_batch_device(d.data_ptr(), len(clips), ft.data_ptr())
    torch.cuda.synchronize()
    want = np.stack([oracle.mfcc_nocmvn(c, om.cfg).reshape(-1) for c in clips[-8:]])
    assert np.isfinite(want).all() and differing(mf[-8:].cpu().numpy(), want) == 0, (name, differing(mf[-8:].cpu().numpy(), want), want.size)
    assert differing(ft.cpu().numpy(), fo) == 0, name
    s2 = torch.zeros((len(clips), gm.n_labels), dtype=torch.float32, device="cuda:0")
    gm.cmvn_inference_batch_device(mf.data_ptr(), len(clips), s2.data_ptr())
    torch.cuda.synchronize()
    assert (bits(s2.cpu().numpy()) == bits(so)).all(), name
    with pytest.raises(pkg.KwsError):
        gm.set_mode(pkg.MODE_FAST)                                  # the fast kernel is built for the tuned configurations only
    gm.close()


@pytest.mark.parametrize("name", sorted(G.REFUSED))
def test_refused_shapes_are_refused_on_the_device_too(name, pkg):
    with pytest.raises(pkg.KwsError) as e:
        pkg.Model(blob=G.blob(name))
    assert e.value.code == -18 and G.REFUSED[name][1] in str(e.value), (name, str(e.value))


@pytest.mark.parametrize("name", G.FLOAT_PCM)
def test_float_pcm_through_run_classifier(name, pkg, oracle, shipped, tmp_path):
    """The SDK's run_classifier() hands the kernels float samples (the F32IN builds: no pair loads, no int16 conversion).  The samples are
    int16 / 32768 exactly, so the int8 graph's scores are the oracle's bits."""
    om = OracleModel(oracle, G.write_model(name, tmp_path))
    gm = pkg.Model(blob=om.blob)
    assert gm.mfcc_kernel == G.SERVED[name][1]
    clip = oracle.synth(8, 0, 1, om.raw_sample_count)[0]
    want = om.run_batch(clip[None])[0]
    buf = clip.astype(np.float32) / np.float32(32768)

    @pkg.GET_DATA_FN
    def get_data(offset, length, out):
        ctypes.memmove(out, buf[offset:offset + length].ctypes.data, 4 * length)
        return 0
    try:
        gm.set_default()
        res = pkg.result_struct(gm.n_labels)()
        sig = pkg.Signal(get_data=get_data, total_length=om.raw_sample_count)
        assert pkg.lib().run_classifier(ctypes.byref(sig), ctypes.byref(res), False) == 0
        got = np.float32([res.classification[i].value for i in range(gm.n_labels)])
        assert (bits(got) == bits(want)).all(), (name, got, want)
    finally:
        shipped.set_default()
        gm.close()


@pytest.mark.parametrize("mode,switch,names", [("scratch", "KWS_DEV_GENERIC_SCRATCH", G.FORCED_SCRATCH), ("cmvn_global", "KWS_DEV_CMVN_GLOBAL", G.FORCED_CMVN_GLOBAL)],
                         ids=["scratch", "cmvn_global"])
def test_forced_forms_at_small_shapes_in_a_fresh_process(mode, switch, names):
    """The scratch kernel and the global-memory cmvnw at shapes the library would not put there (tests/general_envelope_worker.py, on the
    development build, one child at a time): the switches are read once per process, so not in this one."""
    worker = os.path.join(ROOT, "tests", "general_envelope_worker.py")
    out = subprocess.run([sys.executable, worker, mode] + list(names), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300,
                         env=dict(os.environ, **{switch: "1"}))
    assert out.returncode == 0 and "shapes OK" in out.stdout, out.stdout[-2000:] + out.stderr[-3000:]
