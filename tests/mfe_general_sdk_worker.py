"""Child process of tests/test_gpu_mfe_general.py (a fresh process: the SDK's continuous mode keeps a never-reset `first_run` static, like
the reference): run_classifier() on 1 s windows and on 0.5 s windows, and run_classifier_continuous(), with the MFE-block model of shape A
(98 x 40, tests/mfe_general_shapes.py) -- a general plan -- against the oracle.  Exit status 0 = all equal."""
import ctypes
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402,F401
from __graft_entry__ import load_package  # noqa: E402
import mfe_general_shapes as G  # noqa: E402
from kws_testlib import Oracle, OracleModel, bits  # noqa: E402
import continuous_geometry as cg  # noqa: E402

import tempfile  # noqa: E402

pkg = load_package()
o = Oracle()
tmp = tempfile.mkdtemp()
om = OracleModel(o, G.write_model("A", tmp))
gm = pkg.Model(blob=om.blob)
assert gm.mfcc_kernel == G.SPECTRAL["A"]
gm.set_default()
L = pkg.lib()
L.run_classifier_continuous.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_bool]
Result = pkg.result_struct(gm.n_labels)
cur = {}


def get_data(offset, length, out):
    if offset + length > len(cur["s"]):
        return -1
    seg = cur["s"][offset:offset + length].astype(np.float32) / np.float32(32768)
    ctypes.memmove(out, seg.ctypes.data, 4 * length)
    return 0


cb = pkg.GET_DATA_FN(get_data)
clips = np.concatenate([o.synth(51, 0, 3), np.zeros((1, 16000), np.int16)])
want = om.run_batch(clips)
for n in (16000, 8000):                                        # run_classifier: the model's window, and a window of another length
    for i, c in enumerate(clips):
        cur["s"] = c[:n]
        sig, res = pkg.Signal(cb, n), Result()
        rc = L.run_classifier(ctypes.byref(sig), ctypes.byref(res), False)
        got = np.float32([res.classification[j].value for j in range(gm.n_labels)])
        if n == 16000:
            w = want[i]
        else:                                                  # extract_mfe_features of the shorter window, the rest of the input tensor 0
            feat = np.zeros(om.n_features, np.float32)
            part = o.extract_mfe(c[:n], om.cfg)
            feat[:part.size] = part
            w = om.dequantize(om.nn_invoke(om.quantize_input(feat)))
        assert rc == 0 and (bits(got) == bits(w)).all(), ("run_classifier", n, i, got, w)
SLICE = 3999                                                   # a slice of 4000 samples would end inside a frame (frames overlap by half)
audio = o.synth(52, 0, 2).reshape(-1)
want, bad, _ = cg.oracle_scan(om, audio[:6 * SLICE], SLICE)   # the oracle's walk; a slice's last frame may read on into the recording
assert bad is None
L.run_classifier_init()
n_produced = 0
for k in range(6):
    cur["s"] = audio[k * SLICE:(k + 1) * SLICE + 320]            # the application's buffer runs on: a grown slice's last frame reads one sample past the slice
    sig, res = pkg.Signal(cb, SLICE), Result()
    rc = L.run_classifier_continuous(ctypes.byref(sig), ctypes.byref(res), False)
    assert rc == 0, (k, rc)
    if bool(res.classification[0].label):
        got = np.float32([res.classification[j].value for j in range(gm.n_labels)])
        assert (bits(got) == bits(want[n_produced])).all(), ("continuous", k, got, want[n_produced])
        n_produced += 1
assert n_produced == len(want) == 3
print("mfe general sdk worker: %d windows, 6 slices OK" % (2 * len(clips)))
