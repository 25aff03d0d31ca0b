"""Child process of tests/test_gpu_general_envelope.py (a fresh process: KWS_DEV_GENERIC_SCRATCH and KWS_DEV_CMVN_GLOBAL are read once per
process, by the development build of the library only):

    general_envelope_worker.py scratch|cmvn_global <shape of tests/general_dsp_shapes.py> ...

With the matching switch set by the parent, each shape's features, int8 tensor, scores and cepstra before cmvnw must be the oracle's, bit
for bit, on the table's batch; under `scratch` the plan must name kws_spectral_generic_kernel.  (That `cmvn_global` really launches
kws_cmvn_generic_kernel is what tests/test_general_envelope_host.py reads from the launch log.)  Exit status 0 = all equal."""
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402,F401
from __graft_entry__ import load_package  # noqa: E402
import general_dsp_shapes as G  # noqa: E402
from kws_testlib import Oracle, OracleModel, bits  # noqa: E402

mode, names = sys.argv[1], sys.argv[2:]
SWITCH = {"scratch": "KWS_DEV_GENERIC_SCRATCH", "cmvn_global": "KWS_DEV_CMVN_GLOBAL"}[mode]
assert os.environ.get(SWITCH) == "1" and names, "the parent sets %s=1 and names the shapes" % SWITCH
pkg = load_package(dev=True)
assert pkg.LIB_PATH.endswith("_dev.so"), pkg.LIB_PATH
o = Oracle()
tmp = tempfile.mkdtemp()
for name in names:
    om = OracleModel(o, G.write_model(name, tmp))
    gm = pkg.Model(blob=om.blob)
    assert gm.mfcc_kernel == (G.SCRATCH if mode == "scratch" else G.SERVED[name][1]), (name, gm.mfcc_kernel)
    clips = G.clips(o, om.raw_sample_count, 28)
    so, fo, qo = om.run_batch(clips, want_features=True)
    assert np.isfinite(fo).all(), name
    for B in (len(clips), 1):
        s, f, q = gm.run_classifier_batch(clips[-B:], want_features=True)
        assert (bits(f) == bits(fo[-B:])).all(), (name, B, int((bits(f) != bits(fo[-B:])).sum()))
        assert (q == qo[-B:]).all() and (bits(s) == bits(so[-B:])).all(), (name, B)
    d = torch.from_numpy(clips).to("cuda:0")
    mf = torch.zeros((len(clips), gm.n_features), dtype=torch.float32, device="cuda:0")
    gm.mfcc_batch_device(d.data_ptr(), len(clips), mf.data_ptr())
    torch.cuda.synchronize()
    want = np.stack([o.mfcc_nocmvn(c, om.cfg).reshape(-1) for c in clips[-8:]])
    assert (bits(mf[-8:].cpu().numpy()) == bits(want)).all(), name
    s2 = torch.zeros((len(clips), gm.n_labels), dtype=torch.float32, device="cuda:0")
    gm.cmvn_inference_batch_device(mf.data_ptr(), len(clips), s2.data_ptr())
    torch.cuda.synchronize()
    assert (bits(s2.cpu().numpy()) == bits(so)).all(), name
    gm.close()
print("general envelope worker: %s, %d shapes OK" % (mode, len(names)))
