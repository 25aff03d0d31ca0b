"""Child process of tests/test_oracle_vs_reference.py::test_continuous_mode_at_other_slicings (a fresh process per slicing: the reference's
first_run, feature matrix and slice offset are static to the process, and its first step must be the process's first): the compiled
reference's run_classifier_continuous (oracle/_ref, eiref_continuous) and the oracle's kwso_continuous_step driven with the same audio at
one slicing, across one run_classifier_init.  The reference's get_data refuses reads past the slice, so the oracle's end-of-signal is
NULL (0).  usage: continuous_ref_worker.py slice_samples n_slices.  Exit status 0 = every produced flag equal and every score bit-identical."""
import ctypes as C
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from kws_testlib import MODELS, Oracle, OracleModel, Reference, bits  # noqa: E402
from scan_testlib import speech  # noqa: E402

sl, n_slices = int(sys.argv[1]), int(sys.argv[2])
o = Oracle()
om = OracleModel(o, os.path.join(MODELS, "l476_no_yes.kwsm"))
ref = Reference()
audio = speech(o, 900 + sl % 97, sl * n_slices)
audio[sl * (n_slices // 2):sl * (n_slices // 2) + 3 * sl] = 0           # a stretch of digital silence
h = o.L.kwso_continuous_create(om.h)
ref.L.eiref_continuous_init()
so, sr = np.zeros(om.n_labels, np.float32), np.zeros(ref.n_labels, np.float32)
po, pr = C.c_int(), C.c_int()
produced = 0
for k in range(n_slices):
    x = np.ascontiguousarray(audio[k * sl:(k + 1) * sl])
    rc_r = ref.L.eiref_continuous(x.ctypes.data, x.size, sr.ctypes.data, C.byref(pr), None)
    rc_o = o.L.kwso_continuous_step(h, x.ctypes.data, x.size, None, so.ctypes.data, C.byref(po))
    assert rc_r == 0 and rc_o == 0, (sl, k, rc_r, rc_o)
    assert pr.value == po.value, (sl, k, pr.value, po.value)
    if pr.value:
        produced += 1
        assert (bits(sr) == bits(so)).all(), (sl, k, sr, so)
o.L.kwso_continuous_free(h)
print("continuous ref worker: slice %d, %d slices, %d windows OK" % (sl, n_slices, produced))
