"""Graphs with DEPTHWISE_CONV_2D steps on the step trunks without a GPU: the oracle pinned against the compiled reference on every tensor of
every DW_SPECS graph and its float twin; the fixture tests/golden/dwres_graphs.npz (written from the REFERENCE's outputs by tools/make_golden_dwres.py:
what pins the oracle where the reference is absent); the non-vacuity of the graphs; the geometry the table promises; kws_create on the stub runtime
(tests/sanitize: every graph loads, the refusals answer -18 -- the two older "depthwise" refusals included --, mutated blobs never crash);
tools/synth_model.py's blobs of before (SHA-256 digests recorded from the parent commit's generator) and its "dw" step."""
import hashlib
import os
import sys

import numpy as np
import pytest

import conv2d_testlib as C2
import dense_testlib as D
import dwres_testlib as T
import residual_testlib as R
import strided_testlib as S
from kws_testlib import ROOT, SYNTH_SPECS, synth_model_blob
from test_residual_graphs_host import _load_rcs

sys.path.insert(0, os.path.join(ROOT, "tools"))
import dequantize_model  # noqa: E402
import eon_import  # noqa: E402

NAMES = list(T.DW_SPECS)


@pytest.fixture(scope="module")
def oracle_out(oracle):
    """per graph: the oracle's tensors on res_features() (int8 graph) and res_twin_features() (float twin), computed once, shared"""
    out = {}
    for name in NAMES:
        q, taps, out_q, scores = T.oracle_int8(oracle, T.dw_blob(name), T.res_features())
        ftaps, fscores = T.oracle_f32(oracle, T.dw_twin(name), T.res_twin_features())
        out[name] = dict(q=q, taps=taps, out_q=out_q, scores=scores, ftaps=ftaps, fscores=fscores)
    return out


@pytest.mark.parametrize("name", NAMES)
def test_oracle_matches_reference_on_every_tensor(name, oracle, reference):
    """every tensor of the graph, every input, int8 graph and float twin: bit for bit, NaN by position"""
    bad = 0
    blob, twin = T.dw_blob(name), T.dw_twin(name)
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


@pytest.mark.parametrize("name", NAMES)
def test_oracle_reproduces_the_reference_fixture(name, oracle_out):
    """the fixture holds the REFERENCE's output rows (int8 graph: the int8 output tensor; twin: bit patterns) and one digest per step output, hidden
    tensor and logits"""
    g = np.load(T.GOLDEN_DWRES)
    r = oracle_out[name]
    ids = T.tensor_ids(T.dw_blob(name))
    assert np.array_equal(r["out_q"], g[name + "/scores"])
    assert T.same_bits_nan_by_position(r["fscores"], g[name + "/fscores"].view(np.float32))
    dig = [D.digest(r["taps"][i]) for i in ids] + [D.digest(T.canonical_nan(r["ftaps"][i])) for i in ids]
    assert dig == [int(v) for v in g[name + "/digests"]]


def test_fixture_is_small_and_complete():
    assert os.path.getsize(T.GOLDEN_DWRES) < 256 * 1024
    g = np.load(T.GOLDEN_DWRES)
    for name in NAMES:
        assert name + "/scores" in g and name + "/fscores" in g and name + "/digests" in g


@pytest.mark.parametrize("name", NAMES)
def test_graphs_are_not_vacuous(name, oracle_out):
    r = oracle_out[name]
    T.check_not_vacuous(name, T.dw_blob(name), r["taps"], r["out_q"], r["fscores"])


def test_act_ignored_holds_values_below_the_zero_point(oracle_out):
    """dw_act_ignored: the depthwise step has a fused ReLU and an output tensor at zero point 0.  The int8 op ignores the activation
    (depthwise_conv.cc:618-620), so its output holds negative values -- at least 5 % of it --; the float twin honours it: nothing below 0"""
    blob = T.dw_blob("dw_act_ignored")
    tens, nodes, _, _, _ = eon_import.parse_blob(blob)
    dw = [nd for nd in nodes if nd["op"] == 6][0]
    o = dw["out"][0]
    assert dw["p"][3] == 1 and tens[o]["zero"] == [0]
    v = oracle_out["dw_act_ignored"]["taps"][o]
    assert float(np.mean(v < 0)) >= 0.05 and (v > 0).any()
    f = oracle_out["dw_act_ignored"]["ftaps"][o][:T.N_STD]
    assert not (f < 0).any() and (f > 0).any()


def test_table_covers_the_geometries():
    """the shapes and mechanisms the table promises, as the blobs' own tensors and nodes state them"""
    for name in NAMES:
        for blob in (T.dw_blob(name), T.dw_twin(name)):
            tens, nodes, _, _, _ = eon_import.parse_blob(blob)
            assert [tuple(tens[i]["dims"][1:]) for i in T.step_outputs(blob)] == T.GEOMETRY[name], name
            assert len([nd for nd in nodes if nd["op"] == 2 and not tens[nd["in"][0]]["const"] and not tens[nd["in"][1]]["const"]]) == T.N_ADDS[name]
            assert len([nd for nd in nodes if nd["op"] == 6]) == T.N_DW[name] > 0
            for nd in nodes:
                if nd["op"] == 6:
                    w, x, y = tens[nd["in"][1]], tens[nd["in"][0]], tens[nd["out"][0]]
                    assert w["dims"][0] == 1 and w["dims"][3] == y["dims"][3] == x["dims"][3] * nd["p"][6] and nd["p"][6] >= 1

    def parts(name):
        tens, nodes, _, _, _ = eon_import.parse_blob(T.dw_blob(name))
        return tens, nodes, [nd for nd in nodes if nd["op"] == 6]
    # one tensor, two consumers with different margins: a 9-tap depthwise step and a 1 x 1 convolution read c0
    t, n, d = parts("mbx_block")
    c0 = n[1]["out"][0]
    readers = [nd for nd in n if nd["in"][0] == c0]
    assert [nd["op"] for nd in readers] == [6, 1] and t[readers[0]["in"][1]]["dims"] == [1, 1, 9, 16] and t[readers[1]["in"][1]]["dims"] == [16, 1, 1, 16]
    # no ADD at all, a 2-D input image
    t, n, d = parts("ds2d_plain")
    assert T.N_ADDS["ds2d_plain"] == 0 and t[n[0]["out"][0]]["dims"] == [1, 49, 13, 1]
    # multipliers: 8 on one channel, 2 on thirteen
    t, n, d = parts("dw_in_m8")
    assert d[0]["p"][6] == 8 and t[d[0]["in"][0]]["dims"][3] == 1 and d[0]["in"][0] == n[0]["out"][0]
    t, n, d = parts("dw_m2_13")
    assert d[0]["p"][6] == 2 and t[d[0]["in"][0]]["dims"] == [1, 1, 49, 13] and t[d[0]["out"][0]]["dims"][3] == 26
    # an even SAME filter; a strided VALID one under a SAME pool whose last windows are clipped
    t, n, d = parts("dw_k4_same")
    assert t[d[0]["in"][1]]["dims"] == [1, 4, 4, 4] and d[0]["p"][0] == 1
    t, n, d = parts("dw_s2_pool_ragged")
    pool = [nd for nd in n if nd["op"] == 3][0]
    assert d[0]["p"][:3] == [2, 2, 2] and pool["in"][0] == d[0]["out"][0] and pool["p"][:5] == [1, 2, 2, 2, 2]
    assert t[d[0]["out"][0]]["dims"] == [1, 23, 5, 8] and (12 - 1) * 2 + 2 > 23 and (3 - 1) * 2 + 2 > 5
    # the last step; no bias; one filter scale; the bounds
    t, n, d = parts("dw_last")
    assert [nd["op"] for nd in n][-4:] == [6, 0, 4, 5]
    assert len(parts("dw_no_bias")[2][0]["in"]) == 2 and len(parts("dw_last")[2][0]["in"]) == 3
    t, n, d = parts("dw_per_tensor")
    assert len(t[d[0]["in"][1]]["scale"]) == 1
    t, n, d = parts("dw_last")
    assert len(t[d[0]["in"][1]]["scale"]) == 8 and t[d[0]["in"][1]]["qdim"] == 3
    t, n, d = parts("dw_oc64_k16")
    assert t[d[0]["in"][1]]["dims"] == [1, 1, 16, 64]


# ---- kws_create on the stub runtime ----------------------------------------------------------------------------------------------------------

def _bias_minus_one(blob):
    """the no-bias depthwise node as a three-input node whose third input is -1"""
    tens, nodes, t_in, t_out, meta = eon_import.parse_blob(blob)
    dw = [nd for nd in nodes if nd["op"] == 6][0]
    assert len(dw["in"]) == 2
    dw["in"] = list(dw["in"]) + [-1]
    return eon_import.serialise(tens, nodes, t_in, t_out, meta)


def test_every_graph_and_twin_loads(host_exe, tmp_path):
    blobs = {}
    for name in NAMES:
        blobs[name] = T.dw_blob(name)
        blobs[name + "_f32"] = T.dw_twin(name)
    blobs["no_bias_m1"] = _bias_minus_one(T.dw_blob("dw_no_bias"))
    blobs["no_bias_m1_f32"] = _bias_minus_one(T.dw_twin("dw_no_bias"))
    rcs = _load_rcs(host_exe, tmp_path, blobs)
    assert all(rc == 0 for rc in rcs.values()), {k: v for k, v in rcs.items() if v}


def test_refusals(host_exe, tmp_path):
    """KWS_ERROR_UNSUPPORTED_MODEL (-18) for what DESIGN 4.18 leaves out, one blob per refusal (tests/test_gpu_dwres_graphs.py reads the messages), and
    for the blobs of the two older "depthwise" refusals, which only flip a CONV_2D's op code"""
    blobs = dict(T.refused_blobs())
    for key in ("depthwise", "depthwise_f32"):
        blobs["res_" + key] = R.refused_blobs()[key]
        blobs["c2_" + key] = C2.refused_blobs()[key]
    rcs = _load_rcs(host_exe, tmp_path, blobs)
    assert all(rc == -18 for rc in rcs.values()), rcs


def test_mutated_blobs_never_crash(host_exe, tmp_path):
    """160 mutated mbx_block / mnv2_ir / dw_in_m8 / dw_s2_pool_ragged blobs (int8 and twin alternating): a depthwise node's inputs, its options (the depth
    multiplier among them), its filter's dims, any tensor's dims, scales overwritten with 0, -1, 2^30, 2^31 - 1 and small values.  kws_create answers 0 or
    a negative code for each; the program (ASan + UBSan, signed overflow included) never dies"""
    rng = np.random.default_rng(20261021)
    values = [0, -1, 2 ** 30, 2 ** 31 - 1, -2 ** 31, 1, 2, 3, 4, 5, 7, 8, 9, 13, 16, 17, 24, 49, 64, 65, 1024, 1025, 4097, 65536]
    blobs = {}
    k = 0
    while len(blobs) < 160:
        name = ("mbx_block", "mnv2_ir", "dw_in_m8", "dw_s2_pool_ragged")[k % 4]
        base = T.dw_twin(name) if (k // 4) & 1 else T.dw_blob(name)
        tens, nodes, t_in, t_out, meta = eon_import.parse_blob(base)
        tens = [dict(t, dims=list(t["dims"]), scale=list(t["scale"])) for t in tens]
        nodes = [dict(nd, **{"in": list(nd["in"]), "out": list(nd["out"]), "p": list(nd["p"])}) for nd in nodes]
        dws = [nd for nd in nodes if nd["op"] == 6]
        nd = dws[int(rng.integers(len(dws)))]
        kind = k % 6
        k += 1
        if kind == 0:                                    # a node input: any id around the table, -1 and past the end included
            nd["in"][int(rng.integers(len(nd["in"])))] = int(rng.integers(-2, len(tens) + 2))
        elif kind == 1:                                  # an option: padding, strides, activation, dilations, the depth multiplier
            nd["p"][int(rng.integers(7))] = int(rng.choice(values))
        elif kind == 2:                                  # a filter dim (the data keeps its size: the parser or the planner must notice)
            tens[nd["in"][1]]["dims"][int(rng.integers(4))] = int(rng.choice(values))
        elif kind == 3:                                  # a dim of its input or output tensor
            t = tens[nd["in"][0] if rng.integers(2) else nd["out"][0]]
            t["dims"][int(rng.integers(len(t["dims"])))] = int(rng.choice(values))
        elif kind == 4:                                  # a CONV_2D becomes a DEPTHWISE_CONV_2D, or the other way round
            cv = [x for x in nodes if x["op"] in (1, 6)]
            x = cv[int(rng.integers(len(cv)))]
            x["op"] = 7 - x["op"]
        else:                                            # a scale: 0, negative, NaN, huge, tiny
            t = tens[nd["in"][1] if rng.integers(2) else nd["out"][0]]
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
# SHA-256 of synth_model_blob(**spec) as the parent commit's tools/synth_model.py (no "dw" step kind) produced it
from test_conv2d_graphs_host import PARENT_BLOB_SHA256_MORE  # noqa: E402
from test_residual_graphs_host import PARENT_CONV2D_SHA256  # noqa: E402
from test_strided_graphs_host import PARENT_BLOB_SHA256  # noqa: E402

PARENT_RESIDUAL_SHA256 = {
    "tc_identity": "4b4819a760a13fcbd4aeb23272a78c5e619210f935533b21a70705c4b10a43b9",
    "tc_proj_s2": "96ae8ba63ef674068a10493f8d1697693052674fd7292d228a03b1364776d57a",
    "tc_res8": "82437784047bb44763852bc6147a86a21add3ff8258bf5e30a1c7ad1f0a70e6b",
    "id_chain2": "57a7a986d820201b1af860df4bb85a44e7b4dc7d54d5b917f315a085dfa7d815",
    "input_skip": "bb7f15cc98223f13e83ddd38bb390f726e7c3189479674a8e707982d9ddbe3a2",
    "add_self": "19ec66ae72e437a18a40bd4a0707adfda936c32512bc56233a7f9d8e22d74ba2",
    "shortcut_first": "a814f614755b28642c85f5a84d8c18d1d21e55c6d6e9270ebac3964cc3cb5614",
    "add_pool_same": "22c4a802f9ddbcf7e560fdf983c42fb9d419ab9cfc368892d8426c396937357e",
    "tc_pool_keras": "8e312764dbc1f6f36facd80d9955203636f73bedd27b1902b0ce53c5068f076c",
    "narrow_out": "edceb70f466f5fe85ea01615e1c0edb7ef0c5ecc8e404944d185227ec42b2022",
    "oc1": "6c337700148dc810f4c4b405fdf6ed1b2b0eb85bd52025e004e06495c6aa57ce",
    "per_tensor": "a251698abb167ab7ed3d0751bfd8904730e988bd5e15ed9349642f7698096506",
    "zp_edges": "991d25cf7888fb678dac46ab32b30637285633265a453124f7fc4af60c3779d6",
    "slots4": "93fa2db4bdb02983a0c471f97ffac47a550404a8ce7ab261c456728f76f14e04",
    "hidden": "d5e40ee8030a30f0a15b0a9cfa3b791d4bd630aab3b852848d829500dac4f790",
    "res2d_identity": "a9f82fb5effd61a3e86f531d9edb013d7e456373862204f4c260af49bcc8f649",
    "res2d_proj_s2": "5d75454746daf13a51ac514484ee59cb4f5201c4770d086957a65e7844400798",
    "all_pairs_a": "8355b08919a0083e6c11e52051bdcc28b5b1cf0e8939d40066fa932dde11f1d5",
    "all_pairs_b": "ccb5aa0b9c2c636445ad48bbc17fab4b9deb2edf40920683d9abb25038ece66f",
    "all_pairs_c": "8b67851088ca1f8d4e8a02c2e73eb59318713387723f629a2a2fff7b8a92a5d6",
}


def test_synth_model_blobs_are_the_ones_of_before():
    for name, spec in SYNTH_SPECS.items():
        assert hashlib.sha256(synth_model_blob(**spec)).hexdigest() == PARENT_BLOB_SHA256[name], name
    for key, want in PARENT_BLOB_SHA256_MORE.items():
        kind, name = key.split("/")
        blob = S.strided_blob(name) if kind == "strided" else D.dense_blob(name)
        assert hashlib.sha256(blob).hexdigest() == want, key
    for name, want in PARENT_CONV2D_SHA256.items():
        assert hashlib.sha256(C2.conv2d_blob(name)).hexdigest() == want, name
    assert set(PARENT_RESIDUAL_SHA256) == set(R.RES_SPECS)
    for name, want in PARENT_RESIDUAL_SHA256.items():
        assert hashlib.sha256(R.res_blob(name)).hexdigest() == want, name


def test_float_forward_runs_the_depthwise_step(oracle):
    """tools/synth_model.py float_forward (calibration only) against the oracle's float kernels: same shapes, values to float32 rounding -- 2-D and 1-D
    depthwise steps, multipliers 1, 2 and 8, a missing bias"""
    import synth_model
    for name in ("mnv2_ir", "ds2d_plain", "dw_in_m8", "dw_m2_13", "dw_k4_same", "dw_s2_pool_ragged", "dw_no_bias", "mbx_block"):
        tens, nodes, t_in, t_out, _ = eon_import.parse_blob(T.dw_blob(name))
        f = T.res_features()[:8]
        _, fscores = T.oracle_f32(oracle, T.dw_twin(name), f)
        act = synth_model.float_forward(tens, nodes, t_in, f.astype(np.float64))
        assert act[t_out].shape == fscores.shape
        assert np.abs(act[t_out] - fscores).max() < 1e-4, name


def test_the_command_line_spells_a_dw_step(tmp_path):
    """tools/synth_model.py --residual with a dw step and --two-d writes the blob synth_model_blob gives for the same steps"""
    import subprocess
    out = os.path.join(str(tmp_path), "g.kwsm")
    steps = "c0,conv,in,8,3,3,2x2,0,1;d,dw,c0,1,3,3,1x1,0,1;p,conv,d,8,1,1,1x1,0,1"
    subprocess.run([sys.executable, os.path.join(ROOT, "tools", "synth_model.py"), out, "--seed", "1010", "--two-d", "--residual", steps], check=True,
                   stdout=subprocess.PIPE)
    assert open(out, "rb").read() == synth_model_blob(seed=1010, two_d=True, residual=T._SMALL)


def test_tools_pass_such_graphs_through():
    """tools/dequantize_model.py and tools/eon_import.py need no change: the twin keeps dims, node inputs and options (the depth multiplier among them),
    every tensor float32 (shape operands stay int32), and parse / serialise round-trips both blobs"""
    for name in ("mnv2_ir", "dw_no_bias", "dw_m2_13"):
        blob, twin = T.dw_blob(name), T.dw_twin(name)
        tens, nodes, _, _, _ = eon_import.parse_blob(blob)
        ft, fn, _, _, _ = eon_import.parse_blob(twin)
        assert [t["dims"] for t in ft] == [t["dims"] for t in tens] and [(nd["op"], nd["in"], nd["p"]) for nd in fn] == [(nd["op"], nd["in"], nd["p"]) for nd in nodes]
        assert all(t["type"] == 1 or (t["type"] == 2 and t["const"] and len(t["dims"]) == 1 and not t["scale"]) for t in ft)
        for b in (blob, twin):
            assert eon_import.serialise(*eon_import.parse_blob(b)) == b
