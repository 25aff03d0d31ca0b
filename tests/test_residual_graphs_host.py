"""Residual graphs without a GPU: the oracle pinned against the compiled reference on every tensor of every RES_SPECS graph and its float
twin, and on all 65 536 int8 operand pairs of the ADD; the non-vacuity of the graphs; the geometry the table promises; the fixture
tests/golden/residual_graphs.npz (written from the REFERENCE's outputs by tools/make_golden_residual.py: what pins the oracle where the reference is
absent); kws_create on the stub runtime (tests/sanitize: every graph loads, the refusals answer -18, mutated blobs never crash, everything served before
still loads); tools/synth_model.py's blobs of before (SHA-256 digests recorded from the parent commit's generator) and its two-tensor ADD."""
import hashlib
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import conv2d_testlib as C2
import dense_testlib as D
import residual_testlib as T
import strided_testlib as S
from kws_testlib import MODELS, ROOT, SYNTH_SPECS, synth_model_blob

sys.path.insert(0, os.path.join(ROOT, "tools"))
import dequantize_model  # noqa: E402
import eon_import  # noqa: E402

NAMES = list(T.RES_SPECS)


@pytest.fixture(scope="module")
def oracle_out(oracle):
    """per graph: the oracle's tensors on res_features() (int8 graph) and res_twin_features() (float twin), computed once, shared"""
    out = {}
    for name in NAMES:
        q, taps, out_q, scores = T.oracle_int8(oracle, T.res_blob(name), T.res_features())
        ftaps, fscores = T.oracle_f32(oracle, T.res_twin(name), T.res_twin_features())
        out[name] = dict(q=q, taps=taps, out_q=out_q, scores=scores, ftaps=ftaps, fscores=fscores)
    return out


@pytest.fixture(scope="module")
def pairs_out(oracle):
    """per all_pairs graph: the oracle's tensors on all_pairs_rows()"""
    return {name: T.oracle_int8(oracle, T.res_blob(name), q=T.all_pairs_rows()) for name in T.ALL_PAIRS}


@pytest.mark.parametrize("name", NAMES)
def test_oracle_matches_reference_on_every_tensor(name, oracle, reference):
    """every tensor of the graph, every input, int8 graph and float twin: bit for bit, NaN by position"""
    bad = 0
    blob, twin = T.res_blob(name), T.res_twin(name)
    m, mf = D.oracle_model(oracle, blob), D.oracle_model(oracle, twin)
    for row in T.res_features():
        x = m.quantize_input(row)
        r_out, r_t = reference.graph_run(blob, x)
        o_out, o_t = m.nn_invoke(x, taps=True)
        bad += not np.array_equal(o_out, r_out)
        for a, b in zip(o_t, r_t):
            if a.size and b.size:
                bad += not np.array_equal(np.ascontiguousarray(a).view(np.uint8)[:b.nbytes], np.ascontiguousarray(b).view(np.uint8))
    for row in T.res_twin_features():
        r_out, r_t = reference.graph_run(twin, row)
        o_out, o_t = mf.nn_invoke_f32(row, taps=True)
        bad += not T.same_bits_nan_by_position(o_out, r_out)
        for a, b in zip(o_t, r_t):
            if a.size and b.size and b.dtype == np.float32:
                bad += not T.same_bits_nan_by_position(a[:b.size], b)
    assert bad == 0


@pytest.mark.parametrize("name", T.ALL_PAIRS)
def test_oracle_matches_reference_on_all_operand_pairs(name, reference, pairs_out):
    """the ADD output and the output tensor of the all_pairs graphs on all_pairs_rows(): the oracle equals the compiled reference, row by row"""
    blob = T.res_blob(name)
    q, taps, out_q, _ = pairs_out[name]
    add_id = T.step_outputs(blob)[1]
    bad = 0
    for k, row in enumerate(q):
        r_out, r_t = reference.graph_run(blob, row)
        bad += not (np.array_equal(r_out, out_q[k]) and np.array_equal(r_t[add_id], taps[add_id][k]))
    assert bad == 0


@pytest.mark.parametrize("name", T.ALL_PAIRS)
def test_all_pairs_graphs_send_every_operand_pair_through_the_add(name, pairs_out):
    """from the oracle's tensors: the rotating convolution copies the bytes (its output at channel c is the input at channel c + 1), and the ADD's two
    operands take all 65 536 (a, b) values over all_pairs_rows(); the fixture holds the reference's digests of the ADD output and the output rows"""
    blob = T.res_blob(name)
    q, taps, out_q, _ = pairs_out[name]
    rot_id, add_id = T.step_outputs(blob)
    a = q.reshape(len(q), T.H, T.W)
    b = taps[rot_id].reshape(len(q), T.H, T.W)
    assert np.array_equal(b, np.roll(a, -1, axis=2))
    seen = np.zeros((256, 256), bool)
    seen[a.astype(np.int32).ravel() + 128, b.astype(np.int32).ravel() + 128] = True
    assert seen.all()
    tens, nodes, _, _, _ = eon_import.parse_blob(blob)
    ad = [nd for nd in nodes if nd["op"] == 2][0]
    assert tens[ad["in"][0]]["zero"] == tens[ad["in"][1]]["zero"]                    # equal zero points, the ratio the table promises
    ratio = {"all_pairs_a": 1.0, "all_pairs_b": 16.0, "all_pairs_c": 1.0 / 3.7}[name]
    assert abs(tens[ad["in"][1]]["scale"][0] / tens[ad["in"][0]]["scale"][0] / ratio - 1.0) < 1e-6
    g = np.load(T.GOLDEN_RESIDUAL)
    assert [D.digest(taps[add_id]), D.digest(out_q)] == [int(v) for v in g[name + "/pairs"]]


@pytest.mark.parametrize("name", NAMES)
def test_graphs_are_not_vacuous(name, oracle_out):
    r = oracle_out[name]
    T.check_not_vacuous(name, T.res_blob(name), r["taps"], r["out_q"], r["fscores"])


def test_table_covers_the_geometries():
    """the shapes and mechanisms the table promises, as the blobs' own tensors and nodes state them"""
    for name in NAMES:
        for blob in (T.res_blob(name), T.res_twin(name)):
            tens, nodes, _, _, _ = eon_import.parse_blob(blob)
            assert [tuple(tens[i]["dims"][1:]) for i in T.step_outputs(blob)] == T.GEOMETRY[name], name
            assert len([nd for nd in nodes if nd["op"] == 2 and not tens[nd["in"][0]]["const"] and not tens[nd["in"][1]]["const"]]) == T.N_ADDS[name] > 0

    def parts(name):
        tens, nodes, _, _, _ = eon_import.parse_blob(T.res_blob(name))
        return tens, [nd for nd in nodes if nd["op"] == 1], [nd for nd in nodes if nd["op"] == 2], [nd for nd in nodes if nd["op"] == 3]
    # two consumers of one tensor with different padding and stride: a 9-tap stride-2 convolution and a 1 x 1 stride-2 one read c0
    t, c, a, _ = parts("tc_proj_s2")
    assert c[1]["in"][0] == c[3]["in"][0] == c[0]["out"][0] and t[c[1]["in"][1]]["dims"][2] == 9 and t[c[3]["in"][1]]["dims"][2] == 1
    assert c[1]["p"][1] == c[3]["p"][1] == 2 and a[0]["in"] == [c[2]["out"][0], c[3]["out"][0]]
    # the shortcut listed first, and first in the ADD
    t, c, a, _ = parts("shortcut_first")
    assert t[c[1]["in"][1]]["dims"][2] == 1 and a[0]["in"] == [c[1]["out"][0], c[3]["out"][0]]
    assert len(parts("tc_res8")[1]) + len(parts("tc_res8")[2]) == 13 and np.prod(T.GEOMETRY["tc_res8"][-1]) == 336
    # a skip that is a previous ADD's output; the staged input as an operand; the same tensor twice; an even filter
    t, c, a, _ = parts("id_chain2")
    assert a[1]["in"][0] == a[0]["out"][0] and a[1]["p"][0] == 3
    t, c, a, _ = parts("input_skip")
    nodes = eon_import.parse_blob(T.res_blob("input_skip"))[1]
    assert a[0]["in"][1] == nodes[0]["out"][0] == c[0]["in"][0] and a[0]["p"][0] == 0
    t, c, a, _ = parts("add_self")
    assert a[0]["in"][0] == a[0]["in"][1] and a[0]["p"][0] == 2 and t[c[0]["in"][1]]["dims"][2] == 2
    # pools: behind an ADD, SAME with a ragged last window; through the [1][W][1][C] renaming
    t, c, a, p = parts("add_pool_same")
    assert p[0]["in"][0] == a[0]["out"][0] and p[0]["p"][:5] == [1, 2, 1, 3, 1] and c[0]["p"][0] == 2 and (24 - 1) * 2 + 3 > 47
    t, c, a, p = parts("tc_pool_keras")
    assert t[p[0]["in"][0]]["dims"] == [1, 49, 1, 16] and p[0]["p"][:5] == [1, 1, 2, 1, 2]
    # quantisation: per-tensor weights, operand zero points at both ends, a narrow ADD output
    assert len(parts("per_tensor")[0][parts("per_tensor")[1][0]["in"][1]]["scale"]) == 1 and len(parts("tc_proj_s2")[0][parts("tc_proj_s2")[1][0]["in"][1]]["scale"]) == 16
    t, c, a, _ = parts("zp_edges")
    assert [t[i]["zero"][0] for i in a[0]["in"]] == [-128, 127]
    # four live tensors; a hidden layer; the 2-D shapes
    t, c, a, _ = parts("slots4")
    assert a[0]["in"] == [c[1]["out"][0], c[3]["out"][0]] and a[1]["in"] == [c[0]["out"][0], a[0]["out"][0]]
    assert len([nd for nd in eon_import.parse_blob(T.res_blob("hidden"))[1] if nd["op"] == 4]) == 2
    t, c, a, p = parts("res2d_proj_s2")
    assert (c[0]["p"][2], c[0]["p"][1]) == (c[2]["p"][2], c[2]["p"][1]) == (2, 2) and p[0]["p"][:5] == [2, 2, 3, 2, 3]
    assert np.prod(T.GEOMETRY["res2d_identity"][-1]) == 416 and T.GEOMETRY["oc1"][0] == (1, 13, 1)


def test_fixture_is_small_and_complete():
    assert os.path.getsize(T.GOLDEN_RESIDUAL) < 256 * 1024
    g = np.load(T.GOLDEN_RESIDUAL)
    for name in NAMES:
        assert name + "/scores" in g and name + "/fscores" in g and name + "/digests" in g
        assert (name + "/pairs" in g) == (name in T.ALL_PAIRS)


@pytest.mark.parametrize("name", NAMES)
def test_oracle_reproduces_the_reference_fixture(name, oracle_out):
    """the fixture holds the REFERENCE's output rows (int8 graph: the int8 output tensor; twin: bit patterns) and one digest per step output, hidden
    tensor and logits"""
    g = np.load(T.GOLDEN_RESIDUAL)
    r = oracle_out[name]
    ids = T.tensor_ids(T.res_blob(name))
    assert np.array_equal(r["out_q"], g[name + "/scores"])
    assert T.same_bits_nan_by_position(r["fscores"], g[name + "/fscores"].view(np.float32))
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


def test_every_residual_graph_and_twin_loads(host_exe, tmp_path):
    blobs = {}
    for name in NAMES:
        blobs[name] = T.res_blob(name)
        blobs[name + "_f32"] = T.res_twin(name)
    rcs = _load_rcs(host_exe, tmp_path, blobs)
    assert all(rc == 0 for rc in rcs.values()), {k: v for k, v in rcs.items() if v}


def test_refusals(host_exe, tmp_path):
    """KWS_ERROR_UNSUPPORTED_MODEL (-18) for what DESIGN 4.17 leaves out, one blob per refusal (tests/test_gpu_residual_graphs.py reads the messages)"""
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
    for name in C2.CONV2D_SPECS:
        blobs["c_" + name] = C2.conv2d_blob(name)
    rcs = _load_rcs(host_exe, tmp_path, blobs)
    assert all(rc == 0 for rc in rcs.values()), {k: v for k, v in rcs.items() if v}
    # the 2-D family's refusal of a per-channel ADD stays what it was (the graph has no tensor + tensor ADD: it is not residual)
    assert _load_rcs(host_exe, tmp_path, {"c2_add": C2.refused_blobs()["add"]}) == {"c2_add": -18}


def test_mutated_blobs_never_crash(host_exe, tmp_path):
    """200 mutated tc_proj_s2 / id_chain2 / res2d_identity / tc_pool_keras blobs (int8 and twin alternating).  Node inputs: out of range, negative, a later
    node's output, the node's own output, a tensor with two producers; dims, strides, filter sides, pool options overwritten with 0, -1, 2^30, 2^31 - 1 and
    small values; scales 0, negative, NaN.  kws_create answers 0 or a negative code for each; the program (ASan + UBSan, signed overflow included) never
    dies"""
    rng = np.random.default_rng(20261020)
    values = [0, -1, 2 ** 30, 2 ** 31 - 1, -2 ** 31, 1, 2, 3, 4, 5, 7, 8, 13, 16, 17, 49, 64, 65, 1024, 1025, 4097, 65536]
    blobs = {}
    k = 0
    while len(blobs) < 200:
        name = ("tc_proj_s2", "id_chain2", "res2d_identity", "tc_pool_keras")[k % 4]
        base = T.res_twin(name) if (k // 4) & 1 else T.res_blob(name)
        tens, nodes, t_in, t_out, meta = eon_import.parse_blob(base)
        tens = [dict(t, dims=list(t["dims"]), scale=list(t["scale"])) for t in tens]
        nodes = [dict(nd, **{"in": list(nd["in"]), "out": list(nd["out"]), "p": list(nd["p"])}) for nd in nodes]
        convs, pools = [nd for nd in nodes if nd["op"] == 1], [nd for nd in nodes if nd["op"] == 3]
        steps = [nd for nd in nodes if nd["op"] in (1, 2, 3)]
        kind = k % 9
        k += 1
        if kind == 0:                                    # a node input: any id around the table, -1 and past the end included
            nd = steps[int(rng.integers(len(steps)))]
            nd["in"][int(rng.integers(min(2, len(nd["in"]))))] = int(rng.integers(-2, len(tens) + 2))
        elif kind == 1:                                  # ... a LATER node's output
            j = int(rng.integers(len(steps) - 1))
            steps[j]["in"][0] = steps[int(rng.integers(j + 1, len(steps)))]["out"][0]
        elif kind == 2:                                  # ... the node's own output
            nd = steps[int(rng.integers(len(steps)))]
            nd["in"][int(rng.integers(min(2, len(nd["in"]))))] = nd["out"][0]
        elif kind == 3:                                  # a tensor with two producers
            j = int(rng.integers(1, len(steps)))
            steps[j]["out"][0] = steps[int(rng.integers(j))]["out"][0]
        elif kind == 4:                                  # a filter dim (the data keeps its size: the parser or the planner must notice)
            t = tens[convs[int(rng.integers(len(convs)))]["in"][1]]
            t["dims"][int(rng.integers(4))] = int(rng.choice(values))
        elif kind == 5:                                  # a stride / dilation / padding / activation of a convolution, or an ADD's activation
            nd = steps[int(rng.integers(len(steps)))]
            nd["p"][int(rng.integers(6))] = int(rng.choice(values))
        elif kind == 6 and pools:                        # a pool's padding, stride, window or activation
            pools[int(rng.integers(len(pools)))]["p"][int(rng.integers(6))] = int(rng.choice(values))
        elif kind == 7:                                  # a dim of any tensor
            t = tens[int(rng.integers(len(tens)))]
            t["dims"][int(rng.integers(len(t["dims"])))] = int(rng.choice(values))
        else:                                            # a scale: 0, negative, NaN, huge, tiny
            t = tens[int(rng.integers(len(tens)))]
            if not t["scale"]:
                continue
            t["scale"][int(rng.integers(len(t["scale"])))] = float(rng.choice([0.0, -0.05, np.nan, np.inf, 1e-38, 1e30, 1e-9, 3.0]))
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


# ---- tools/synth_model.py ----------------------------------------------------------------------------------------------------------------------
# SHA-256 of synth_model_blob(**spec) as the parent commit's tools/synth_model.py (no residual=) produced it
from test_conv2d_graphs_host import PARENT_BLOB_SHA256_MORE  # noqa: E402
from test_strided_graphs_host import PARENT_BLOB_SHA256  # noqa: E402

PARENT_CONV2D_SHA256 = {
    "ei_2d": "c52586ac9c496c0ebf5fdf54ca3ee258d7a73b60566dc0c6577576bafceb5a65",
    "acts": "d6e8fa86794d7326fd282412f0bb5fd4d3bd007a6b59fe5e07cc3a07bf2a0ba5",
    "hidden": "8d40e015146fe83c1db005960a31374933c6f0a386a93047583f99ede72cd1c3",
    "in_zp_127": "e383e661436eff24c3612f70903678944b606d9320ea3a9ce22ffd5a7f810af0",
}


def test_synth_model_blobs_are_the_ones_of_before():
    for name, spec in SYNTH_SPECS.items():
        assert hashlib.sha256(synth_model_blob(**spec)).hexdigest() == PARENT_BLOB_SHA256[name], name
        assert hashlib.sha256(synth_model_blob(**spec, residual=None, two_d=False)).hexdigest() == PARENT_BLOB_SHA256[name], name
    for key, want in PARENT_BLOB_SHA256_MORE.items():
        kind, name = key.split("/")
        blob = S.strided_blob(name) if kind == "strided" else D.dense_blob(name)
        assert hashlib.sha256(blob).hexdigest() == want, key
    for name, want in PARENT_CONV2D_SHA256.items():
        assert hashlib.sha256(C2.conv2d_blob(name)).hexdigest() == want, name


def test_float_forward_runs_the_two_tensor_add(oracle):
    """tools/synth_model.py float_forward (calibration only) against the oracle's float kernels on residual graphs: same shapes, values to float32
    rounding"""
    import synth_model
    for name in ("tc_proj_s2", "id_chain2", "add_pool_same", "tc_pool_keras", "res2d_proj_s2", "input_skip"):
        tens, nodes, t_in, t_out, _ = eon_import.parse_blob(T.res_blob(name))
        assert synth_model.is_residual(tens, nodes)
        f = T.res_features()[:8]
        _, fscores = T.oracle_f32(oracle, T.res_twin(name), f)
        act = synth_model.float_forward(tens, nodes, t_in, f.astype(np.float64))
        assert act[t_out].shape == fscores.shape
        assert np.abs(act[t_out] - fscores).max() < 1e-4, name


def test_dequantize_model_makes_the_float_twin():
    """tools/dequantize_model.py on a residual blob needs no change: every tensor float32 (shape operands stay int32), dims, node inputs and options kept"""
    tens, nodes, _, _, _ = eon_import.parse_blob(T.res_blob("tc_pool_keras"))
    ft, fn, _, _, _ = eon_import.parse_blob(dequantize_model.dequantize(T.res_blob("tc_pool_keras")))
    assert [t["dims"] for t in ft] == [t["dims"] for t in tens] and [(nd["in"], nd["p"]) for nd in fn] == [(nd["in"], nd["p"]) for nd in nodes]
    assert all(t["type"] == 1 or (t["type"] == 2 and t["const"] and len(t["dims"]) == 1 and not t["scale"]) for t in ft)
