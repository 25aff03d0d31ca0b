"""Strided and dilated temporal convolutions without a GPU: the oracle pinned against the compiled reference on every STRIDED_SPECS graph
and its float twin, the pinned disagreement on SAME-padded dilated depthwise (why it stays refused), the non-vacuity of the graphs, the fixture
tests/golden/strided_graphs.npz (written from the REFERENCE's outputs by tools/make_golden_strided.py: what pins the oracle where the reference is
absent), kws_create on the stub runtime (tests/sanitize: every graph loads, the refusals answer -18, mutated strides and dilations never crash) and
tools/synth_model.py's blobs of before (SHA-256 digests recorded from the parent commit's generator)."""
import hashlib
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import dense_testlib as D
import strided_testlib as S
from kws_testlib import MODELS, ROOT, SYNTH_SPECS, synth_model_blob

sys.path.insert(0, os.path.join(ROOT, "tools"))
import dequantize_model  # noqa: E402
import eon_import  # noqa: E402

NAMES = list(S.STRIDED_SPECS)


@pytest.fixture(scope="module")
def oracle_out(oracle):
    """per graph: the oracle's tensors on strided_features(), int8 graph and float twin (computed once, shared)"""
    out = {}
    for name in NAMES:
        f = S.strided_features(name)
        q, taps, out_q, scores = D.oracle_int8(oracle, S.strided_blob(name), f)
        ftaps, fscores = S.oracle_f32_blocks(oracle, S.strided_twin(name), f)
        out[name] = dict(q=q, taps=taps, out_q=out_q, scores=scores, ftaps=ftaps, fscores=fscores)
    return out


def _tensor_mismatches(name, oracle, reference, rows):
    """tensors (over rows, int8 graph and twin) on which kws_oracle.c and the reference's own op registrations differ in any bit"""
    bad = 0
    for blob, is_float in ((S.strided_blob(name), False), (S.strided_twin(name), True)):
        m = D.oracle_model(oracle, blob)
        for row in rows:
            x = row if is_float else m.quantize_input(row)
            r_out, r_t = reference.graph_run(blob, x)
            o_out, o_t = (m.nn_invoke_f32 if is_float else m.nn_invoke)(x, taps=True)
            bad += not np.array_equal(np.asarray(o_out).view(np.uint8), np.asarray(r_out).view(np.uint8))
            for a, b in zip(o_t, r_t):
                if a.size and b.size:
                    bad += not np.array_equal(np.ascontiguousarray(a).view(np.uint8)[:b.nbytes], np.ascontiguousarray(b).view(np.uint8))
    return bad


@pytest.mark.parametrize("name", NAMES)
def test_oracle_matches_reference_on_every_tensor(name, oracle, reference):
    """bit for bit on EVERY tensor of the graph, every input, int8 and float twin"""
    assert _tensor_mismatches(name, oracle, reference, S.strided_features(name)) == 0


def test_same_padded_dilated_depthwise_disagrees(oracle, reference):
    """The refusal's reason, written down: the reference's DEPTHWISE_CONV_2D computes its padding with dilation 1 (depthwise_conv.cc:489-492) while its
    loops dilate, so a SAME-padded dilated depthwise convolution comes out shifted; the oracle pads with the real dilation.  With VALID padding (spec
    dw_d2_valid, above) the two agree."""
    g = S.conv_geometry(S.strided_blob("dw_d2_same"))[0]
    assert g["depthwise"] and g["dilation"] == 2 and g["padding"] == 1
    assert _tensor_mismatches("dw_d2_same", oracle, reference, S.strided_features("dw_d2_same")[:16]) > 0


def test_table_covers_the_geometries():
    """the shapes the table promises, as the blobs' own tensors state them"""
    def g(name, i=0):
        return S.conv_geometry(S.strided_blob(name))[i]
    pad = lambda k: max(0, (k["out_w"] - 1) * k["stride"] + (k["taps"] - 1) * k["dilation"] + 1 - k["in_w"])
    assert (g("s2_k3")["out_w"], pad(g("s2_k3")) // 2) == (25, 1)
    assert (g("s2_even", 1)["in_w"], g("s2_even", 1)["out_w"], pad(g("s2_even", 1))) == (48, 24, 1)                 # total 1: left 0, right 1
    assert (g("s3_k7_pool")["out_w"], g("s2_valid")["out_w"], g("s5_k2")["out_w"]) == (17, 23, 10)
    k = g("s5_k2")
    assert (k["out_w"] - 1) * k["stride"] + k["taps"] - k["in_w"] == -2
    k = g("d4_wide", 1)
    assert k["in_w"] == 7 and (k["taps"] - 1) * k["dilation"] + 1 == 9
    assert (g("d3_valid")["out_w"], g("dw_d2_valid")["out_w"]) == (37, 45)
    assert [k["out_w"] for k in S.conv_geometry(S.strided_blob("s2_chain"))] == [25, 13, 7]
    assert (g("w98_s2")["in_w"], g("w98_s2")["out_w"]) == (98, 49)
    for name in ("mc_s2", "mc_d2"):
        k = g(name, 1)
        assert (k["in_c"], k["out_c"], k["depthwise"]) == (16, 32, False)
    assert g("c40_s2")["in_c"] == 40
    assert all(S.is_strided(S.strided_blob(n)) for n in NAMES)


def test_float_blocking_classes_are_covered():
    """every (tb, fused) class kws_nn_f32_pick_blocking can return occurs on a strided or dilated block of some twin (restated pick; the GPU test asserts
    the library's own through kws_dev_f32_blocking)"""
    got = {(tb, fused) for n in NAMES for tb, fused, sd in S.f32_blockings(S.strided_twin(n)) if sd}
    assert got == S.BLOCKING_CLASSES


@pytest.mark.parametrize("name", NAMES)
def test_graphs_are_not_vacuous(name, oracle_out):
    r = oracle_out[name]
    S.check_not_vacuous(name, S.strided_blob(name), r["taps"], r["scores"], r["fscores"])


def test_fixture_is_small_and_complete():
    assert os.path.getsize(S.GOLDEN_STRIDED) < 256 * 1024
    g = np.load(S.GOLDEN_STRIDED)
    for name in NAMES:
        assert name + "/scores" in g and name + "/fscores" in g and name + "/digests" in g


@pytest.mark.parametrize("name", NAMES)
def test_oracle_reproduces_the_reference_fixture(name, oracle_out):
    """the fixture holds the REFERENCE's output rows (int8 graph: the int8 output tensor; twin: bit patterns) and one digest per block output, hidden
    tensor and logits"""
    g = np.load(S.GOLDEN_STRIDED)
    r = oracle_out[name]
    _, _, hidden, last, _, _ = D.graph_layout(S.strided_blob(name))
    ids = D.block_outputs(S.strided_blob(name)) + hidden + [last]
    assert np.array_equal(r["out_q"], g[name + "/scores"])
    assert np.array_equal(r["fscores"].view(np.uint32), g[name + "/fscores"].view(np.uint32))
    dig = [D.digest(r["taps"][i]) for i in ids] + [D.digest(r["ftaps"][i]) for i in ids]
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


def test_every_strided_graph_and_twin_loads(host_exe, tmp_path):
    blobs = {}
    for name in NAMES:
        blobs[name] = S.strided_blob(name)
        blobs[name + "_f32"] = S.strided_twin(name)
    rcs = _load_rcs(host_exe, tmp_path, blobs)
    assert all(rc == 0 for rc in rcs.values()), {k: v for k, v in rcs.items() if v}


def _conv(n, k=0):
    return [nd for nd in n if nd["op"] in (1, 6)][k]


def _set_p(idx, value, k=0):
    def f(t, n):
        _conv(n, k)["p"][idx] = value
    return f


def _edit_out_rows(t, n):
    # the strided convolution's output tensor claims the stride-1 width
    y = t[_conv(n)["out"][0]]
    y["dims"][2] = 49
    y["nbytes"] = int(np.prod(y["dims"]))


REFUSED = {
    "stride_h_2": dict(seed=700, blocks=((16, 3, 1),), conv_stride={0: 2}, edit=_set_p(2, 2)),
    "dil_h_2": dict(seed=701, blocks=((16, 3, 1),), conv_stride={0: 2}, edit=_set_p(5, 2)),
    "dw_same_dilated": S.DW_D2_SAME,
    "out_rows": dict(seed=702, blocks=((16, 3, 1),), conv_stride={0: 2}, edit=_edit_out_rows),
    "stride_0": dict(seed=703, blocks=((16, 3, 1),), edit=_set_p(1, 0)),
    "stride_neg": dict(seed=704, blocks=((16, 3, 1),), edit=_set_p(1, -1)),
    "stride_past_rows": dict(seed=705, blocks=((16, 3, 1),), edit=_set_p(1, 50)),
    "stride_2_30": dict(seed=706, blocks=((16, 3, 1),), edit=_set_p(1, 2 ** 30)),
    "dil_0": dict(seed=707, blocks=((16, 3, 1),), edit=_set_p(4, 0)),
    "dil_neg": dict(seed=708, blocks=((16, 3, 1),), edit=_set_p(4, -1)),
    "dil_int_max": dict(seed=709, blocks=((16, 3, 1),), edit=_set_p(4, 2 ** 31 - 1)),
    "dil_4096": dict(seed=710, blocks=((16, 3, 1),), edit=_set_p(4, 4096)),
    # 16 taps at dilation 200 on 49 x 64 channels, un-pooled: a padded image of more than 3000 rows x 64 bytes per wave, past the LDS budget
    "lds": dict(seed=711, blocks=((64, 3, 1), (8, 16, 1)), conv_dilation={1: 200}),
}


def test_refusals(host_exe, tmp_path):
    """KWS_ERROR_UNSUPPORTED_MODEL (-18) for what DESIGN 4.15 leaves out, int8 and float (tests/test_gpu_strided_graphs.py reads the messages)"""
    bad = {k: synth_model_blob(**v) for k, v in REFUSED.items()}
    bad.update({k + "_f32": dequantize_model.dequantize(v) for k, v in list(bad.items())})
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


def test_mutated_strides_and_dilations_never_crash(host_exe, tmp_path):
    """200 mutated s2_d2 / dw_s3_k5_pool blobs (int8 and twin alternating): a stride or dilation of a conv node overwritten (0, -1, 2^30, 2^31 - 1, small
    values), a dim, a tensor index or a node input flipped.  kws_create answers 0 or a negative code for each; the program (ASan + UBSan, signed overflow
    included) never dies"""
    rng = np.random.default_rng(20250611)
    values = [0, -1, 2 ** 30, 2 ** 31 - 1, -2 ** 31, 2, 3, 7, 48, 49, 50, 4095, 4096, 65536]
    blobs = {}
    for k in range(200):
        name = ("s2_d2", "dw_s3_k5_pool")[k & 1]
        base = S.strided_twin(name) if k & 2 else S.strided_blob(name)
        tens, nodes, t_in, t_out, meta = eon_import.parse_blob(base)
        tens = [dict(t, dims=list(t["dims"])) for t in tens]
        nodes = [dict(nd, **{"in": list(nd["in"]), "out": list(nd["out"]), "p": list(nd["p"])}) for nd in nodes]
        convs = [nd for nd in nodes if nd["op"] in (1, 6)]
        kind = k % 5
        if kind in (0, 1):                               # p[1] (stride_w) / p[4] (dilation_width_factor), sometimes both
            nd = convs[int(rng.integers(len(convs)))]
            nd["p"][1 if kind == 0 else 4] = int(rng.choice(values))
            if rng.integers(2):
                nd["p"][4 if kind == 0 else 1] = int(rng.choice(values))
        elif kind == 2:                                  # a dim
            t = tens[int(rng.integers(len(tens)))]
            t["dims"][int(rng.integers(len(t["dims"])))] = int(rng.choice([1, 2, 3, 7, 64, 255, 4097, 65536]))
        elif kind == 3:                                  # a tensor index
            nd = nodes[int(rng.integers(len(nodes)))]
            nd["out"][0] = int(rng.integers(-2, len(tens) + 2))
        else:                                            # a node input
            nd = nodes[int(rng.integers(len(nodes)))]
            nd["in"][int(rng.integers(len(nd["in"])))] = int(rng.integers(-2, len(tens) + 2))
        try:
            blob = eon_import.serialise(tens, nodes, t_in, t_out, meta)
        except Exception:
            blob = base
        while blob == base or blob in blobs.values():    # the serialiser refused, or the draw hit an earlier case: a random stride / dilation instead
            tens2, nodes2, _, _, _ = eon_import.parse_blob(base)
            convs2 = [nd for nd in nodes2 if nd["op"] in (1, 6)]
            nd = convs2[int(rng.integers(len(convs2)))]
            nd["p"] = list(nd["p"])
            nd["p"][int(rng.choice([1, 4]))] = int(rng.integers(-2 ** 31, 2 ** 31))
            blob = eon_import.serialise(tens2, nodes2, t_in, t_out, meta)
        blobs["mut%03d" % k] = blob
    assert len(set(blobs.values())) == 200
    rcs = _load_rcs(host_exe, tmp_path, blobs)
    assert all(rc <= 0 for rc in rcs.values()), rcs
    assert any(rc == 0 for rc in rcs.values()) and any(rc == -18 for rc in rcs.values())       # some mutations stay inside the family, some leave it


# ---- tools/synth_model.py: the blobs of before ------------------------------------------------------------------------------------------------
# SHA-256 of synth_model_blob(**SYNTH_SPECS[name]) as the parent commit's tools/synth_model.py (no conv_stride / conv_dilation) produced it
PARENT_BLOB_SHA256 = {
    "seed1": "1915616126b661b6f54a68ee1797e33719157a5d5284342df9ff663eac7f89e3",
    "seed2": "0abb6400d93dd9573941c9f8fa48cb7f82d2076f9f693e85219dfd25b3e7bfc3",
    "seed4": "59f9bd28d89867f70419c6f69ef45864d4e87ad6b177dfa7160db0838e1a3b18",
    "seed5": "e2ac1a5bb89390d2a2b6f3544e9f7fcb315f43c15d526efa2dca17d2ff0f60d5",
    "seed6": "762cc071d0801b08f69faabbcd6f17d1454c25da323b05b990aaf835b5c49952",
    "seed7": "abdefbb7650b9167956c076ee903dcfdf7c7fd383f9238e73a654f082ac5dc19",
    "f40c40": "6615ea85c4426b4e77c069ffd22540d41cd812ca19f595a2d780afca18094480",
    "dscnn_a": "fd6abc1687677d8a58edf451b621b8045ebc045f6f02df40975b8d51669c7dbd",
    "mfma_mix": "5e9eea5aa9a950c8b9b56104236034e07a12d33311afc069a8d94f093d7aa976",
    "mfma_mix2": "ea4a2fedccf1b6640703b4d76f2cf19b75ebda630fa403c014576f4667dcccc1",
    "ei_default": "784138f80157294b7db212cb9f0c65dfc4de0a36ca6590d1a03116fe237573ad",
    "ei_default_same": "b68c3c1df0b3d24ed08fe3e8cad9e63a681492b848b53919fe8675c2b9d386c6",
    "ei_default40": "6135dab075faa1c832c88b5b7ca879dac6748cdef009ff722bd113ad7f3bb8d4",
    "dscnn_b": "84690d0b41835322c04bd9ae1d32580a4ecb6cfb0907b8a8a6e78da2042076d4",
    "cfg5_dscnn": "91b776a2420343d5795cb6934fe9d397494322f241167d80809d48aa6894f1a6",
}


def test_synth_model_blobs_are_the_ones_of_before():
    assert set(PARENT_BLOB_SHA256) == set(SYNTH_SPECS)
    for name, spec in SYNTH_SPECS.items():
        assert hashlib.sha256(synth_model_blob(**spec)).hexdigest() == PARENT_BLOB_SHA256[name], name
        # ... and stride 1 / dilation 1 spelled out draws nothing either
        nb = len(spec.get("blocks", ((30, 7, 7), (10, 7, 7))))
        explicit = synth_model_blob(**spec, conv_stride={b: 1 for b in range(nb)}, conv_dilation={b: 1 for b in range(nb)})
        assert hashlib.sha256(explicit).hexdigest() == PARENT_BLOB_SHA256[name], name


def test_float_forward_honours_stride_and_dilation(oracle):
    """tools/synth_model.py float_forward (calibration only) against the oracle's float kernels on a strided and dilated graph: same shapes, values to
    float32 rounding"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import synth_model
    twin = S.strided_twin("s2_d2")
    tens, nodes, t_in, t_out, _ = eon_import.parse_blob(S.strided_blob("s2_d2"))
    f = S.strided_features("s2_d2")[:8]
    _, fscores = S.oracle_f32_blocks(oracle, twin, f)
    act = synth_model.float_forward(tens, nodes, t_in, f.astype(np.float64))
    assert act[t_out].shape == fscores.shape
    assert np.abs(act[t_out] - fscores).max() < 1e-4
