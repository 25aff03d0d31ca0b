"""-m gpu: the int8 network kernels at the edges of their quantisation (kws_testlib.QUANT_EDGES), in KWS_MODE_EXACT through
Model.nn_batch: the int8 output, the FULLY_CONNECTED output and EVERY block's pooled tensor equal the restatement's tensors over
384 input rows and the reference's recorded results (tests/golden/quant_edges_l476.npz) on 24 of them; scores bit for bit.
The CPU pins (tests/test_oracle_vs_reference.py, tests/test_oracle_golden.py) hold the restatement to the reference on the same
models and assert that each case tests something."""
import os

import numpy as np
import pytest

from kws_testlib import (QUANT_EDGES, QUANT_EDGE_LABELS, QUANT_REFUSALS, ROOT, OracleModel, bits, quant_edge_blob, quant_edge_digest,
                         quant_edge_golden, quant_edge_golden_rows, quant_edge_groups, quant_edge_inputs, quant_edge_run, synth_model_blob)

pytestmark = pytest.mark.gpu

F32_SCORE_TOL = 1e-6           # the project's bar for exact-mode float32 scores (the float softmax uses the device expf, kws.h)


@pytest.fixture(scope="module")
def pkg():
    import sys
    sys.path.insert(0, ROOT)
    import torch  # noqa: F401  (first: libamdhip64 of the torch wheel is the one the process uses)
    from __graft_entry__ import load_package
    return load_package()


@pytest.fixture(scope="module")
def golden():
    return quant_edge_golden()


def mismatches(got, want):
    """per tensor, how many values differ -- printed by a failing assertion"""
    s, pooled, fc, out = got
    return dict(out=int((out != want["out"]).sum()), fc=int((fc != want["fc"]).sum()), pooled=int((pooled != want["pooled"]).sum()),
                pooled_values=int(pooled.size), scores=int((bits(s) != bits(want["scores"])).sum()))


def check_model(pkg, oracle, tmp_path, key, blob, where, golden, scalar_too):
    """one model: the library's tensors against the restatement's (all rows) and the recorded reference (its rows).  Returns
    (the library's model, the restatement's model, the input rows, the restatement's tensors)"""
    p = tmp_path / "m.kwsm"
    p.write_bytes(blob)
    om = OracleModel(oracle, str(p))
    qs = quant_edge_inputs(om.n_features)
    want = quant_edge_run(lambda q: om.nn_invoke(q, taps=True), blob, where, qs)
    want["scores"] = np.stack([om.dequantize(o) for o in want["out"]])
    rows = quant_edge_golden_rows()
    gm = pkg.Model(blob=blob)                                   # KWS_MODE_EXACT is a model's mode until set_mode says otherwise
    runs = [("default", 0)] + ([("generic kernel", 1)] if scalar_too else [])
    for what, force in runs:
        L = pkg.lib()
        L.kws_dev_force_scalar_nn(force)
        try:
            got = gm.nn_batch(qs)
        finally:
            L.kws_dev_force_scalar_nn(0)
        s, pooled, fc, out = got
        assert pooled.shape == want["pooled"].shape, (key, what)
        d = mismatches(got, want)
        assert d["pooled"] == 0 and d["fc"] == 0 and d["out"] == 0 and d["scores"] == 0, (key, what, d)   # every block, every row
        if golden is not None:
            g = golden[key]
            assert (out[rows] == g["out"]).all() and (fc[rows] == g["fc"]).all(), (key, what)
            assert (quant_edge_digest(pooled[rows]) == g["pooled_sha"]).all(), (key, what)
    return gm, om, qs, want


@pytest.mark.parametrize("group", [g for g in quant_edge_groups() if not g.endswith("/labels")])     # labels: the test below
def test_int8_network_at_quantisation_edges(group, pkg, oracle, golden, tmp_path):
    """Every case of one edited op (a convolution / depthwise / pointwise position, the ADD behind one, the FULLY_CONNECTED, the
    head, the label count) of g2 (two-block matrix-core kernel, 16-byte rows), g2w (the same kernel with 64-byte rows) or gd
    (generic kernel: un-pooled matrix-core blocks, both depthwise paths, a VALID-pooled sdot4 block).  g2 and g2w run a second
    time on the generic kernel (kws_dev_force_scalar_nn), whose pooled sdot4 path they then take."""
    keys = [k for k in sorted(QUANT_EDGES) if k.rsplit("/", 1)[0] == group]
    assert keys
    for key in keys:
        e = QUANT_EDGES[key]
        gm, om, qs, want = check_model(pkg, oracle, tmp_path, key, quant_edge_blob(key), e["where"], golden, e["graph"] in ("g2", "g2w"))
        gm.close()


@pytest.mark.parametrize("graph", ["g2", "gd"])
@pytest.mark.parametrize("n_labels", QUANT_EDGE_LABELS)
def test_label_counts_up_to_the_limit(graph, n_labels, pkg, oracle, golden, tmp_path):
    """13 .. 48 labels (nn_head with n_seg = 1 at 33 and more; lg's 48 ints in the two-block kernel): batches of 1, 3 and 65
    rows, the float32 twin (logits bit for bit, scores within F32_SCORE_TOL), and 48 synthetic clips end to end through
    run_classifier_batch against the restatement's run_classifier."""
    import sys
    import torch
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from dequantize_model import dequantize
    key = "%s/labels/%d" % (graph, n_labels)
    blob = quant_edge_blob(key)
    gm, om, qs, want = check_model(pkg, oracle, tmp_path, key, blob, QUANT_EDGES[key]["where"], golden, graph == "g2")
    assert gm.n_labels == n_labels
    for n in (1, 3, 65):
        s, pooled, fc, out = gm.nn_batch(qs[60:60 + n])
        assert (out == want["out"][60:60 + n]).all() and (fc == want["fc"][60:60 + n]).all(), (key, n)
        assert (pooled == want["pooled"][60:60 + n]).all() and (bits(s) == bits(want["scores"][60:60 + n])).all(), (key, n)
    clips = oracle.synth(48, 0, 48)
    assert (bits(gm.run_classifier_batch(clips)) == bits(om.run_batch(clips))).all(), key
    gm.close()
    bf = dequantize(blob)
    pf = tmp_path / "f.kwsm"
    pf.write_bytes(bf)
    of = OracleModel(oracle, str(pf))
    gf = pkg.Model(blob=bf)
    x = (np.random.default_rng(n_labels).standard_normal((24, of.n_features)) * np.float32(4.0)).astype(np.float32)
    f = torch.from_numpy(x).to("cuda:0")
    s = torch.empty((24, n_labels), dtype=torch.float32, device="cuda:0")
    lg = torch.empty((24, n_labels), dtype=torch.float32, device="cuda:0")
    gf.nn_f32_batch_device(f.data_ptr(), 24, s.data_ptr(), lg.data_ptr())
    torch.cuda.synchronize()
    s, lg = s.cpu().numpy(), lg.cpu().numpy()
    n_t = len(of.tensor_bytes)
    for i in range(24):
        so, taps = of.nn_invoke_f32(x[i], taps=True)
        assert (bits(lg[i]) == bits(taps[n_t - 2])).all(), (key, i)
        assert np.abs(s[i] - so).max() <= F32_SCORE_TOL, (key, i)
    gf.close()


@pytest.mark.parametrize("key", sorted(QUANT_REFUSALS))
def test_models_kws_create_must_refuse(key, pkg):
    """A left shift that can carry (accumulator + bias) past 2^31 -- undefined in the reference, and a requantisation that is no
    longer monotonic, which the kernels' pooling of raw accumulators relies on -- on a pooled conv block, the second block of
    the two-block kernel, a depthwise and a pointwise block; and 49 labels: KWS_ERROR_UNSUPPORTED_MODEL from kws_create."""
    with pytest.raises(pkg.KwsError) as ei:
        pkg.Model(blob=synth_model_blob(**QUANT_REFUSALS[key]))
    assert ei.value.code == -18, key
    if key.startswith("wrap/"):
        assert "block" in str(ei.value) and "channel" in str(ei.value), str(ei.value)      # the refusal names where
