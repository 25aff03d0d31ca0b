"""2-D convolutional graphs without a GPU: the oracle pinned against the compiled reference on every tensor of every CONV2D_SPECS graph and
its float twin, the non-vacuity of the graphs, the geometry the table promises, the fixture tests/golden/conv2d_graphs.npz (written from the REFERENCE's
outputs by tools/make_golden_conv2d.py: what pins the oracle where the reference is absent), kws_create on the stub runtime (tests/sanitize: every graph
loads, the refusals answer -18, mutated blobs never crash, everything served before still loads) and tools/synth_model.py's blobs of before (SHA-256
digests recorded from the parent commit's generator)."""
import hashlib
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import conv2d_testlib as T
import dense_testlib as D
import strided_testlib as S
from kws_testlib import MODELS, ROOT, SYNTH_SPECS, synth_model_blob

sys.path.insert(0, os.path.join(ROOT, "tools"))
import dequantize_model  # noqa: E402
import eon_import  # noqa: E402

NAMES = list(T.CONV2D_SPECS)


@pytest.fixture(scope="module")
def oracle_out(oracle):
    """per graph: the oracle's tensors on conv2d_features() (int8 graph) and conv2d_twin_features() (float twin), computed once, shared"""
    out = {}
    for name in NAMES:
        q, taps, out_q, scores = D.oracle_int8(oracle, T.conv2d_blob(name), T.conv2d_features(name))
        ftaps, fscores = S.oracle_f32_blocks(oracle, T.conv2d_twin(name), T.conv2d_twin_features(name))
        out[name] = dict(q=q, taps=taps, out_q=out_q, scores=scores, ftaps=ftaps, fscores=fscores)
    return out


@pytest.mark.parametrize("name", NAMES)
def test_oracle_matches_reference_on_every_tensor(name, oracle, reference):
    """every tensor of the graph, every input, int8 graph and float twin: bit for bit, NaN by position"""
    bad = 0
    blob, twin = T.conv2d_blob(name), T.conv2d_twin(name)
    m, mf = D.oracle_model(oracle, blob), D.oracle_model(oracle, twin)
    for row in T.conv2d_features(name):
        x = m.quantize_input(row)
        r_out, r_t = reference.graph_run(blob, x)
        o_out, o_t = m.nn_invoke(x, taps=True)
        bad += not np.array_equal(o_out, r_out)
        for a, b in zip(o_t, r_t):
            if a.size and b.size:
                bad += not np.array_equal(np.ascontiguousarray(a).view(np.uint8)[:b.nbytes], np.ascontiguousarray(b).view(np.uint8))
    for row in T.conv2d_twin_features(name):
        r_out, r_t = reference.graph_run(twin, row)
        o_out, o_t = mf.nn_invoke_f32(row, taps=True)
        bad += not T.same_bits_nan_by_position(o_out, r_out)
        for a, b in zip(o_t, r_t):
            if a.size and b.size and b.dtype == np.float32:
                bad += not T.same_bits_nan_by_position(a[:b.size], b)
    assert bad == 0


@pytest.mark.parametrize("name", NAMES)
def test_graphs_are_not_vacuous(name, oracle_out):
    r = oracle_out[name]
    T.check_not_vacuous(name, T.conv2d_blob(name), r["taps"], r["out_q"], r["fscores"])


def test_table_covers_the_geometries():
    """the shapes the table promises, as the blobs' own tensors state them"""
    for name in NAMES:
        assert T.block_shapes(T.conv2d_blob(name)) == T.GEOMETRY[name], name
        assert T.block_shapes(T.conv2d_twin(name)) == T.GEOMETRY[name], name

    def convs(name):
        tens, nodes, _, _, _ = eon_import.parse_blob(T.conv2d_blob(name))
        return tens, [nd for nd in nodes if nd["op"] == 1], [nd for nd in nodes if nd["op"] == 3]
    pad = lambda out, stride, k, size: max(0, (out - 1) * stride + k - size)           # total padding along one axis (kernels/padding.h)
    # asymmetric filters, [out_c][kh][kw][in_c]
    assert convs("k5x3")[0][convs("k5x3")[1][0]["in"][1]]["dims"] == [8, 5, 3, 1] and convs("k3x5")[0][convs("k3x5")[1][0]["in"][1]]["dims"] == [8, 3, 5, 1]
    # the 7 x 7 filter is wider than its 13 x 4 image; the padding (3 + 3) exceeds it
    t, c, _ = convs("k7x7_w4")
    assert t[c[2]["in"][0]]["dims"] == [1, 13, 4, 8] and t[c[2]["in"][1]]["dims"][1:3] == [7, 7] and pad(4, 1, 7, 4) == 6
    # strided: total padding odd on one axis (in front 0, behind 1), even on the other
    t, c, _ = convs("s2x2")
    assert (c[0]["p"][2], c[0]["p"][1]) == (2, 2) and (pad(25, 2, 2, 49), pad(7, 2, 3, 13)) == (1, 2)
    t, c, _ = convs("s1x3")
    assert (c[0]["p"][2], c[0]["p"][1]) == (1, 3) and (pad(49, 1, 3, 49), pad(5, 3, 2, 13)) == (2, 1)
    t, c, _ = convs("s2x1")
    assert (c[0]["p"][0], c[0]["p"][2], c[0]["p"][1]) == (2, 2, 1)                     # the VALID strided case
    # pools: window != stride, one axis only, VALID
    assert convs("pool3s2")[2][0]["p"][:5] == [1, 2, 2, 3, 3]
    assert convs("pool2x1")[2][0]["p"][1:5] == [1, 2, 1, 2] and convs("pool1x2")[2][0]["p"][1:5] == [2, 1, 2, 1]
    assert all(p["p"][0] == 2 for p in convs("valid")[2]) and all(cv["p"][0] == 2 for cv in convs("valid")[1])
    # activations and the missing bias
    t, c, _ = convs("acts")
    assert [cv["p"][3] for cv in c] == [0, 2, 3] and len(c[1]["in"]) == 2
    # per-tensor / per-channel scales, the zero point edges, the dense stack, the wide images
    assert len(convs("per_tensor")[0][convs("per_tensor")[1][0]["in"][1]]["scale"]) == 1 and len(convs("ei_2d")[0][convs("ei_2d")[1][0]["in"][1]]["scale"]) == 8
    assert convs("in_zp_m128")[0][0]["zero"] == [-128] and convs("in_zp_127")[0][0]["zero"] == [127]
    assert len([nd for nd in eon_import.parse_blob(T.conv2d_blob("hidden"))[1] if nd["op"] == 4]) == 2
    assert convs("w40")[0][convs("w40")[1][0]["in"][0]]["dims"] == [1, 49, 40, 1] and convs("mfe98")[0][convs("mfe98")[1][0]["in"][0]]["dims"] == [1, 98, 40, 1]
    assert np.prod(T.GEOMETRY["nopool_chain"][-1]) % 2 == 1                               # an odd-sized hand-off


def test_fixture_is_small_and_complete():
    assert os.path.getsize(T.GOLDEN_CONV2D) < 256 * 1024
    g = np.load(T.GOLDEN_CONV2D)
    for name in NAMES:
        assert name + "/scores" in g and name + "/fscores" in g and name + "/digests" in g


@pytest.mark.parametrize("name", NAMES)
def test_oracle_reproduces_the_reference_fixture(name, oracle_out):
    """the fixture holds the REFERENCE's output rows (int8 graph: the int8 output tensor; twin: bit patterns) and one digest per block output, hidden
    tensor and logits"""
    g = np.load(T.GOLDEN_CONV2D)
    r = oracle_out[name]
    ids = T.tensor_ids(T.conv2d_blob(name))
    assert np.array_equal(r["out_q"], g[name + "/scores"])
    assert T.same_bits_nan_by_position(r["fscores"], g[name + "/fscores"])
    dig = [D.digest(r["taps"][i]) for i in ids] + [D.digest(T.canonical_nan(r["ftaps"][i])) for i in ids]
    assert dig == [int(v) for v in g[name + "/digests"]]


# ---- kws_create on the stub runtime ----------------------------------------------------------------------------------------------------------

def _load_rcs(host_exe, tmp_path, blobs):
    """{name: rc} of kws_create for each blob, in runs of the stub-runtime program (an ASan + UBSan build: it dies on a memory error or an overflow)"""
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
        for line in r.stdout.splitlines():
            m = re.match(r"^(\S+\.kwsm) rc (-?\d+)$", line)
            if m:
                rcs[os.path.basename(m.group(1))[:-5]] = int(m.group(2))
    assert len(rcs) == len(blobs)
    return rcs


def test_every_conv2d_graph_and_twin_loads(host_exe, tmp_path):
    blobs = {}
    for name in NAMES:
        blobs[name] = T.conv2d_blob(name)
        blobs[name + "_f32"] = T.conv2d_twin(name)
    rcs = _load_rcs(host_exe, tmp_path, blobs)
    assert all(rc == 0 for rc in rcs.values()), {k: v for k, v in rcs.items() if v}


def test_refusals(host_exe, tmp_path):
    """KWS_ERROR_UNSUPPORTED_MODEL (-18) for what DESIGN 4.16 leaves out, one blob per refusal (tests/test_gpu_conv2d_graphs.py reads the messages)"""
    rcs = _load_rcs(host_exe, tmp_path, T.refused_blobs())
    assert all(rc == -18 for rc in rcs.values()), rcs


def test_everything_served_before_still_loads(host_exe, tmp_path):
    blobs = {}
    for fn in sorted(os.listdir(MODELS)):
        if fn.endswith(".kwsm"):
            blobs["m_" + fn[:-5]] = open(os.path.join(MODELS, fn), "rb").read()
    for name, spec in SYNTH_SPECS.items():
        blobs["s_" + name] = synth_model_blob(**spec)
    for name in S.STRIDED_SPECS:
        blobs["t_" + name] = S.strided_blob(name)
    rcs = _load_rcs(host_exe, tmp_path, blobs)
    assert all(rc == 0 for rc in rcs.values()), {k: v for k, v in rcs.items() if v}


def test_mutated_blobs_never_crash(host_exe, tmp_path):
    """200 mutated ei_2d / pool3s2 / s2x2 blobs (int8 and twin alternating): filter dims, strides, pool windows, tensor dims and node inputs overwritten
    with 0, -1, 2^30, 2^31 - 1 and small values.  kws_create answers 0 or a negative code for each; the program (ASan + UBSan, signed overflow included)
    never dies"""
    rng = np.random.default_rng(20260414)
    values = [0, -1, 2 ** 30, 2 ** 31 - 1, -2 ** 31, 1, 2, 3, 4, 5, 7, 8, 13, 49, 64, 65, 1024, 1025, 4097, 65536]
    blobs = {}
    k = 0
    while len(blobs) < 200:
        name = ("ei_2d", "pool3s2", "s2x2")[k % 3]
        base = T.conv2d_twin(name) if k & 1 else T.conv2d_blob(name)
        tens, nodes, t_in, t_out, meta = eon_import.parse_blob(base)
        tens = [dict(t, dims=list(t["dims"])) for t in tens]
        nodes = [dict(nd, **{"in": list(nd["in"]), "out": list(nd["out"]), "p": list(nd["p"])}) for nd in nodes]
        convs, pools = [nd for nd in nodes if nd["op"] == 1], [nd for nd in nodes if nd["op"] == 3]
        kind = k % 5
        k += 1
        if kind == 0:                                    # a filter dim (the data keeps its size: the parser or the planner must notice)
            t = tens[convs[int(rng.integers(len(convs)))]["in"][1]]
            t["dims"][int(rng.integers(4))] = int(rng.choice(values))
        elif kind == 1:                                  # a stride / dilation / padding / activation of a convolution
            convs[int(rng.integers(len(convs)))]["p"][int(rng.integers(6))] = int(rng.choice(values))
        elif kind == 2:                                  # a pool's padding, stride, window or activation
            pools[int(rng.integers(len(pools)))]["p"][int(rng.integers(6))] = int(rng.choice(values))
        elif kind == 3:                                  # a dim of any tensor
            t = tens[int(rng.integers(len(tens)))]
            t["dims"][int(rng.integers(len(t["dims"])))] = int(rng.choice(values))
        else:                                            # a node input or output
            nd = nodes[int(rng.integers(len(nodes)))]
            if rng.integers(2):
                nd["in"][int(rng.integers(len(nd["in"])))] = int(rng.integers(-2, len(tens) + 2))
            else:
                nd["out"][0] = int(rng.integers(-2, len(tens) + 2))
        try:
            for t in tens:                               # nbytes follows the dims where that is possible at all (else the parser refuses the blob)
                if not t["const"] and all(0 < d < 1 << 20 for d in t["dims"]):
                    t["nbytes"] = int(np.prod(t["dims"])) * (1 if t["type"] == 9 else 4)
            blob = eon_import.serialise(tens, nodes, t_in, t_out, meta)
        except Exception:
            continue
        if blob != base and blob not in blobs.values():
            blobs["mut%03d" % len(blobs)] = blob
    rcs = _load_rcs(host_exe, tmp_path, blobs)
    assert all(rc <= 0 for rc in rcs.values()), rcs
    assert any(rc == 0 for rc in rcs.values()) and any(rc == -18 for rc in rcs.values())       # some mutations stay inside the family, some leave it


# ---- tools/synth_model.py: the blobs of before ------------------------------------------------------------------------------------------------
# SHA-256 of synth_model_blob(**spec) as the parent commit's tools/synth_model.py (no blocks2d) produced it: SYNTH_SPECS (the digests
# tests/test_strided_graphs_host.py pins) and four STRIDED_SPECS / DENSE_SPECS graphs that go through the edit / dense / stride paths
from test_strided_graphs_host import PARENT_BLOB_SHA256  # noqa: E402

PARENT_BLOB_SHA256_MORE = {
    "strided/s2_k3": "b26b355bfa8740b1e87263695480d4cffa3c372e4c9d1c3046c004d027947b22",
    "strided/dw_s3_k5_pool": "fd69b88baa13eba5219dd81794ddbf791ee67692dd83ce2db220773fd183fe99",
    "dense/d0_h20_h10": "6281d6b951c82bd639f11857a107527896007bfbb0ddb2516c0e61f29234f789",
    "dense/c1_h48_h16": "59af958809472dbadccca048764416eb746c8e58bc3aad2c4878bdfff0cea311",
}


def test_synth_model_blobs_are_the_ones_of_before():
    for name, spec in SYNTH_SPECS.items():
        assert hashlib.sha256(synth_model_blob(**spec)).hexdigest() == PARENT_BLOB_SHA256[name], name
        assert hashlib.sha256(synth_model_blob(**spec, blocks2d=None)).hexdigest() == PARENT_BLOB_SHA256[name], name
    for key, want in PARENT_BLOB_SHA256_MORE.items():
        kind, name = key.split("/")
        blob = S.strided_blob(name) if kind == "strided" else D.dense_blob(name)
        assert hashlib.sha256(blob).hexdigest() == want, key


def test_float_forward_runs_the_2d_ops(oracle):
    """tools/synth_model.py float_forward (calibration only) against the oracle's float kernels on strided, VALID and oddly pooled 2-D graphs: same shapes,
    values to float32 rounding"""
    import synth_model
    for name in ("ei_2d", "valid", "s2x2", "s1x3", "pool3s2", "k7x7_w4"):
        tens, nodes, t_in, t_out, _ = eon_import.parse_blob(T.conv2d_blob(name))
        f = T.conv2d_features(name)[:8]
        _, fscores = S.oracle_f32_blocks(oracle, T.conv2d_twin(name), f)
        act = synth_model.float_forward(tens, nodes, t_in, f.astype(np.float64))
        assert act[t_out].shape == fscores.shape
        assert np.abs(act[t_out] - fscores).max() < 1e-4, name


def test_dequantize_model_makes_the_float_twin():
    """tools/dequantize_model.py on a 2-D blob: every tensor float32 (shape operands stay int32), dims and node options kept"""
    tens, nodes, _, _, _ = eon_import.parse_blob(T.conv2d_blob("acts"))
    ft, fn, _, _, _ = eon_import.parse_blob(dequantize_model.dequantize(T.conv2d_blob("acts")))
    assert [t["dims"] for t in ft] == [t["dims"] for t in tens] and [nd["p"] for nd in fn] == [nd["p"] for nd in nodes]
    assert all(t["type"] == 1 or (t["type"] == 2 and t["const"] and len(t["dims"]) == 1 and not t["scale"]) for t in ft)
