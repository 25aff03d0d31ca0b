"""kws_create on the models of the quantisation-edge table, without a GPU: the library's host code on the stub HIP runtime of
tests/sanitize (host_exe, tests/conftest.py).  The plan builder refuses a left shift that can overflow; it must refuse nothing else."""
import glob
import os
import subprocess

from kws_testlib import MODELS, QUANT_EDGES, QUANT_REFUSALS, SYNTH_SPECS, quant_edge_blob, random_graph_spec, synth_model_blob


def create_codes(host_exe, tmp_path, blobs):
    """name -> kws_create's return code"""
    paths = {}
    for name, blob in blobs.items():
        paths[name] = str(tmp_path / (name.replace("/", "__") + ".kwsm"))
        with open(paths[name], "wb") as f:
            f.write(blob)
    out = subprocess.run([host_exe] + list(paths.values()), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    rc = {ln.split(" rc ")[0]: int(ln.split(" rc ")[1]) for ln in out.stdout.splitlines() if " rc " in ln}
    return {name: rc[p] for name, p in paths.items()}


def test_plan_builder_accepts_every_edge_model_and_refuses_the_overflowing_ones(host_exe, tmp_path):
    rc = create_codes(host_exe, tmp_path, {k: quant_edge_blob(k) for k in QUANT_EDGES})
    assert [k for k, v in rc.items() if v != 0] == []
    rc = create_codes(host_exe, tmp_path, {k: synth_model_blob(**kw) for k, kw in QUANT_REFUSALS.items()})
    assert rc == {k: -18 for k in QUANT_REFUSALS}


def test_left_shift_bound_refuses_nothing_that_loaded_before(host_exe, tmp_path):
    """the shipped models, the named synthetic graphs and the random graphs of the fuzz tests load as before; and the bound cannot
    have been what refused a random draw: every effective multiplier of every draw is below 1, a right shift or none"""
    import eon_import
    rc = create_codes(host_exe, tmp_path, {k: synth_model_blob(**kw) for k, kw in SYNTH_SPECS.items()})
    assert rc == {k: 0 for k in SYNTH_SPECS}
    shipped = sorted(glob.glob(os.path.join(MODELS, "*.kwsm")))
    out = subprocess.run([host_exe] + shipped, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert out.stdout.count(" rc 0") == len(shipped)
    blobs = {"fz%d" % s: synth_model_blob(**random_graph_spec(s)) for s in range(150) if random_graph_spec(s) is not None}
    rc = create_codes(host_exe, tmp_path, blobs)
    assert sum(v == 0 for v in rc.values()) >= 60 and set(rc.values()) <= {0, -18}, rc
    for name, blob in blobs.items():
        tensors, nodes, _, _, _ = eon_import.parse_blob(blob)
        for nd in nodes:
            if nd["op"] in (1, 4, 6):
                i, w, o = (tensors[t]["scale"] for t in (nd["in"][0], nd["in"][1], nd["out"][0]))
                assert max(w) * i[0] / o[0] < 1.0, name
