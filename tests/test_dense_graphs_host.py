"""Graphs with dense stacks without a GPU: the oracle pinned against the compiled reference on every DENSE_SPECS model and its float
twin, the non-vacuity of those models, the fixture tests/golden/dense_l476.npz (written from the REFERENCE's outputs by tools/make_golden_dense.py:
what pins the oracle where the reference is absent), and kws_create on the stub runtime (tests/sanitize): every model loads, the design limits are
refused, malformed blobs never crash."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import dense_testlib as D
from kws_testlib import MODELS, ROOT, SYNTH_SPECS, have_reference, synth_model_blob

sys.path.insert(0, os.path.join(ROOT, "tools"))
import dequantize_model  # noqa: E402
import eon_import  # noqa: E402

NAMES = list(D.DENSE_SPECS)


@pytest.fixture(scope="module")
def oracle_out(oracle):
    """per model: the oracle's tensors on dense_features(), int8 graph and float twin (computed once, shared)"""
    out = {}
    for name in NAMES:
        f = D.dense_features(name)
        q, taps, out_q, scores = D.oracle_int8(oracle, D.dense_blob(name), f)
        ftaps, fscores = D.oracle_f32(oracle, D.dense_twin(name), f)
        out[name] = dict(q=q, taps=taps, out_q=out_q, scores=scores, ftaps=ftaps, fscores=fscores)
    return out


@pytest.mark.parametrize("name", NAMES)
def test_oracle_matches_reference_on_every_tensor(name, oracle, reference):
    """kws_oracle.c against the reference's own op registrations (Reference.graph_run), bit for bit, on EVERY tensor of the graph: int8 and float twin"""
    f = D.dense_features(name)
    for blob, is_float in ((D.dense_blob(name), False), (D.dense_twin(name), True)):
        m = D.oracle_model(oracle, blob)
        for row in f:
            x = row if is_float else m.quantize_input(row)
            r_out, r_t = reference.graph_run(blob, x)
            o_out, o_t = (m.nn_invoke_f32 if is_float else m.nn_invoke)(x, taps=True)
            assert np.array_equal(np.asarray(o_out).view(np.uint8), np.asarray(r_out).view(np.uint8))
            for i, (a, b) in enumerate(zip(o_t, r_t)):
                if a.size and b.size:
                    assert np.array_equal(np.ascontiguousarray(a).view(np.uint8)[:b.nbytes], np.ascontiguousarray(b).view(np.uint8)), (name, is_float, i)


@pytest.mark.parametrize("name", NAMES)
def test_models_are_not_vacuous(name, oracle_out):
    """a saturated graph gives every clip the same tensor and proves nothing: every hidden tensor takes >= 16 distinct values (one unit: 8), at most
    half of its entries sit on a clamp bound, and the model produces >= 8 distinct score rows"""
    r = oracle_out[name]
    tens, nodes, hidden, last, _, _ = D.graph_layout(D.dense_blob(name))
    D.check_not_vacuous(name, tens, nodes, hidden, r["taps"], r["scores"], r["fscores"])


def test_fixture_is_small_and_complete():
    assert os.path.getsize(D.GOLDEN_DENSE) < 256 * 1024
    g = np.load(D.GOLDEN_DENSE)
    for name in NAMES:
        assert name + "/scores" in g and name + "/fscores" in g and name + "/digests" in g


@pytest.mark.parametrize("name", NAMES)
def test_oracle_reproduces_the_reference_fixture(name, oracle_out):
    """the fixture holds the REFERENCE's score rows (int8: exactly representable; float: bit patterns) and one digest per hidden tensor and logits"""
    g = np.load(D.GOLDEN_DENSE)
    r = oracle_out[name]
    _, _, hidden, last, _, _ = D.graph_layout(D.dense_blob(name))
    assert np.array_equal(r["out_q"], g[name + "/scores"])
    assert np.array_equal(r["fscores"].view(np.uint32), g[name + "/fscores"].view(np.uint32))
    dig = [D.digest(r["taps"][i]) for i in hidden + [last]] + [D.digest(r["ftaps"][i]) for i in hidden + [last]]
    assert dig == [int(v) for v in g[name + "/digests"]]


# ---- kws_create on the stub runtime ----------------------------------------------------------------------------------------------------------

def _load_rcs(host_exe, tmp_path, blobs):
    """{name: rc} of kws_create for each blob, one run of the stub-runtime program (an ASan + UBSan build: it dies on a memory error)"""
    paths = []
    for name, blob in blobs.items():
        p = os.path.join(str(tmp_path), name + ".kwsm")
        with open(p, "wb") as f:
            f.write(blob)
        paths.append(p)
    rcs = {}
    for i in range(0, len(paths), 64):
        r = subprocess.run([host_exe] + paths[i:i + 64], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        for line in r.stdout.splitlines():                 # "<path> rc <code>"; a loaded model's walk through the entry points prints more
            m = re.match(r"^(\S+\.kwsm) rc (-?\d+)$", line)
            if m:
                rcs[os.path.basename(m.group(1))[:-5]] = int(m.group(2))
    assert len(rcs) == len(blobs)
    return rcs


def test_every_dense_model_and_twin_loads(host_exe, tmp_path):
    blobs = {}
    for name in NAMES:
        blobs[name] = D.dense_blob(name)
        blobs[name + "_f32"] = D.dense_twin(name)
    rcs = _load_rcs(host_exe, tmp_path, blobs)
    assert all(rc == 0 for rc in rcs.values()), {k: v for k, v in rcs.items() if v}


def _edit_overflow(t, n):
    # a multiplier of 2^20 on the first layer: (sum|w| * max|x| + |bias|) << 21 passes 2^31 - 1
    fc = [nd for nd in n if nd["op"] == 4][0]
    t[fc["in"][1]]["scale"] = [float(np.float32(t[fc["out"][0]]["scale"][0] / t[fc["in"][0]]["scale"][0] * 2.0 ** 20))]


def _edit_chain_mismatch(t, n):
    # the second layer's weights claim 21 inputs for a 20-unit layer in front
    fc = [nd for nd in n if nd["op"] == 4][1]
    w = t[fc["in"][1]]
    units = w["dims"][0]
    w["dims"] = [units, 21]
    w["nbytes"] = units * 21
    w["data"] = bytes(units * 21)


def test_design_limits_are_refused(host_exe, tmp_path):
    bad = {
        "five_layers": synth_model_blob(seed=400, blocks=(), dense=((8, 1), (8, 1), (8, 1), (8, 1))),
        "units_257": synth_model_blob(seed=401, blocks=(), dense=((257, 1),)),
        "inputs_4097": synth_model_blob(seed=402, blocks=(), ncep=17, num_filters=32, raw_samples=77440, dense=((8, 1),)),
        "left_shift": synth_model_blob(seed=403, blocks=(), dense=((20, 1), (10, 1)), edit=_edit_overflow),
        "chain": synth_model_blob(seed=404, blocks=(), dense=((20, 1), (10, 1)), edit=_edit_chain_mismatch),
    }
    tens, _, t_in, _, _ = eon_import.parse_blob(bad["inputs_4097"])
    assert tens[t_in]["dims"][1] == 4097
    bad.update({k + "_f32": dequantize_model.dequantize(v) for k, v in list(bad.items()) if k != "left_shift"})
    rcs = _load_rcs(host_exe, tmp_path, bad)
    assert all(rc == -18 for rc in rcs.values()), rcs


def test_models_served_before_still_load(host_exe, tmp_path):
    blobs = {}
    for fn in sorted(os.listdir(MODELS)):
        if fn.endswith(".kwsm"):
            blobs["m_" + fn[:-5]] = open(os.path.join(MODELS, fn), "rb").read()
    for name, spec in SYNTH_SPECS.items():
        blobs["s_" + name] = synth_model_blob(**spec)
    rcs = _load_rcs(host_exe, tmp_path, blobs)
    assert all(rc == 0 for rc in rcs.values()), {k: v for k, v in rcs.items() if v}


def test_malformed_blobs_never_crash(host_exe, tmp_path):
    """200 mutated or truncated d0_h20_h10 / c2_h64 blobs: a dim, a byte count, a tensor index or a node input flipped, or the tail cut off.
    kws_create answers 0 or a negative code for each; the program (ASan + UBSan) never dies"""
    rng = np.random.default_rng(20250117)
    blobs = {}
    for k in range(200):
        base = D.dense_blob(("d0_h20_h10", "c2_h64")[k & 1])
        tens, nodes, t_in, t_out, meta = eon_import.parse_blob(base)
        tens, nodes = [dict(t) for t in tens], [dict(nd, **{"in": list(nd["in"]), "out": list(nd["out"]), "p": list(nd["p"])}) for nd in nodes]
        kind = k % 5
        if kind == 0:                                    # a dim
            t = tens[int(rng.integers(len(tens)))]
            t["dims"] = list(t["dims"])
            t["dims"][int(rng.integers(len(t["dims"])))] = int(rng.choice([1, 2, 3, 7, 64, 255, 4097, 65536]))
        elif kind == 1:                                  # a byte count (data follows it where the tensor is constant)
            t = tens[int(rng.integers(len(tens)))]
            t["nbytes"] = max(0, t["nbytes"] + int(rng.choice([-4, -1, 1, 4, 1000])))
            if t["const"]:
                t["data"] = bytes(t["nbytes"])
        elif kind == 2:                                  # a tensor index
            nd = nodes[int(rng.integers(len(nodes)))]
            nd["out"][0] = int(rng.integers(-2, len(tens) + 2))
        elif kind == 3:                                  # a node input
            nd = nodes[int(rng.integers(len(nodes)))]
            nd["in"][int(rng.integers(len(nd["in"])))] = int(rng.integers(-2, len(tens) + 2))
        try:
            blob = eon_import.serialise(tens, nodes, t_in, t_out, meta)
        except Exception:
            # a mutation the serialiser itself refuses: a byte of the blob's body flipped instead
            b2 = bytearray(base)
            b2[int(rng.integers(64, len(base)))] ^= int(rng.integers(1, 256))
            blob = bytes(b2)
        if kind == 4:                                    # truncated
            blob = base[:int(rng.integers(8, len(base)))]
        while blob == base or blob in blobs.values():    # the draw hit the value that was there, or an earlier case: a flipped byte instead
            b2 = bytearray(base)
            b2[int(rng.integers(64, len(base)))] ^= int(rng.integers(1, 256))
            blob = bytes(b2)
        blobs["mut%03d" % k] = blob
    assert len(set(blobs.values())) == 200               # 200 different blobs, none of them a base blob
    rcs = _load_rcs(host_exe, tmp_path, blobs)
    assert all(rc <= 0 for rc in rcs.values()), rcs
