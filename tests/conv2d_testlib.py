"""Named 2-D convolutional graphs (CONV_2D + MAX_POOL_2D with both spatial axes live, in front of a dense stack) shared by
tests/test_conv2d_graphs_host.py, tests/test_gpu_conv2d_graphs.py, tools/make_golden_conv2d.py and tools/gpu_conv2d_rate.py: each an int8 graph with a
calibrated head and its float32 twin (tools/dequantize_model.py).  49 x 13 features and the shipped DSP block unless a spec says otherwise, 4 labels.  The
shapes are the smallest at which each thing can go wrong."""
import functools
import os

import numpy as np

import dense_testlib as D
import strided_testlib as S
from kws_testlib import GOLDEN, synth_model_blob

GOLDEN_CONV2D = os.path.join(GOLDEN, "conv2d_graphs.npz")
N_STD = 40               # rows every graph and twin is run on: 32 standardised random rows, 7 past both ends of the input quantisation, one all-zero row
N_FLOAT = 8              # rows of the float twins alone: signed zeros, subnormals, FLT_MAX neighbours, +inf, NaN
INPUT_SEED = 6262


def _calibration_rows(n_features, mfe):
    """what the DSP block hands the network: standardised columns (cmvnw), or -- the MFE block -- values in [0, 1]"""
    rng = np.random.default_rng(78)
    return rng.uniform(0.0, 1.0, (256, n_features)) if mfe else rng.standard_normal((256, n_features))


def _lift(mfe=False, per_tensor=False, in_zp=None):
    """The edit every spec ends with (it draws nothing from the model's generator).  As drawn, a block's ReLU parks about half of its outputs on the bound and
    the drawn output scales saturate the rest; a test on such a graph proves little.  Block by block, on 256 calibration rows: a ReLU / ReLU6 convolution's
    int32 bias is set per channel so that the float twin's pre-activation has mean 0.7 x its own deviation (about a quarter of the outputs below zero), a
    ReLU6 / ReLU_N1_TO_1 convolution's weight scales so that the pre-activations' deviation is 1.5 / 0.5; then the hidden layers, the activation ranges and
    the head are calibrated (tools/synth_model.py).  per_tensor: every filter gets ONE scale first.  in_zp: the input tensor's zero point is set first, and
    the calibration rows are what that quantisation lets through."""
    sm = D.synth_model

    def edit(t, n):
        x = _calibration_rows(t[0]["dims"][1], mfe)
        if in_zp is not None:
            for tid in (0, n[0]["out"][0]):              # the input tensor and its RESHAPE (which must keep the quantisation)
                t[tid]["zero"] = [in_zp]
            s = t[0]["scale"][0]
            x = ((np.round(x / s) + in_zp + 128) % 256 - 128 - in_zp) * s     # (the reference's input quantisation wraps, ei_run_classifier.h:436-444)
        for idx, nd in enumerate(n):
            if nd["op"] != 1:
                continue
            tw = t[nd["in"][1]]
            tb = t[nd["in"][2]] if len(nd["in"]) > 2 and nd["in"][2] >= 0 else None
            in_scale = t[nd["in"][0]]["scale"][0]
            if per_tensor:
                tw["scale"], tw["zero"] = [float(np.float32(np.mean(tw["scale"])))], [0]
            act = nd["p"][3]
            a = sm.float_forward(t, n[:idx], 0, x)[nd["in"][0]]
            nd["p"][3] = 0                                   # the pre-activation: this node without its clamp and bias
            if tb is not None:
                tb["data"] = bytes(len(tb["data"]))
            if act in (2, 3):
                pre = sm.float_forward(t, [nd], nd["in"][0], a)[nd["out"][0]]
                tw["scale"] = [float(np.float32(s_ * (1.5 if act == 3 else 0.5) / pre.std())) for s_ in tw["scale"]]
            pre = sm.float_forward(t, [nd], nd["in"][0], a)[nd["out"][0]]
            pre = pre.reshape(-1, pre.shape[-1])
            nd["p"][3] = act
            if tb is not None:
                tb["scale"] = [float(np.float32(in_scale) * np.float32(s_)) for s_ in tw["scale"]]
                tb["zero"] = [0] * len(tb["scale"])
                lift = 0.7 * pre.std(axis=0) if act in (1, 3) else 0.0
                tb["data"] = np.round((lift - pre.mean(axis=0)) / np.float64(tb["scale"])).astype(np.int32).tobytes()
            sm.calibrate_ranges(t, n[:idx + 1], 0, x)
        fcs = [nd for nd in n if nd["op"] == 4]
        sm.calibrate_hidden(t, n, 0, fcs[:-1], x)
        sm.calibrate_head(t, n, 0, fcs[-1]["in"][1], fcs[-1]["in"][2], fcs[-1]["out"][0], 1.5, 0, x=x)
    return edit


_EI = ((8, 3, 3, 2), (16, 3, 3, 2))
_K5X3 = ((8, 5, 3, 2), (8, 3, 3, 2))
_M40 = dict(num_filters=40, ncep=40, low=300, high=0)
CONV2D_SPECS = {
    # the stock graph: 49 x 13 -> 25 x 7 -> 13 x 4, both pools with a ragged last window on both axes
    "ei_2d": dict(seed=801, blocks2d=_EI, edit=_lift()),
    # asymmetric filters: a swap of the axes anywhere shows
    "k5x3": dict(seed=802, blocks2d=_K5X3, edit=_lift()),
    "k3x5": dict(seed=803, blocks2d=((8, 3, 5, 2), (8, 3, 3, 2)), edit=_lift()),
    "k1x1": dict(seed=804, blocks2d=((8, 3, 3, 2), (12, 1, 1, 1)), edit=_lift()),                                  # pointwise behind a 3 x 3 block
    # 7 x 7 SAME on 13 x 4: the filter is wider than the image and the padding (3 + 3) exceeds it
    "k7x7_w4": dict(seed=805, blocks2d=((8, 3, 3, 2), (8, 3, 3, 2), (8, 7, 7, 1)), edit=_lift()),
    # VALID convolutions and VALID pools: 49 x 13 -> 47 x 11 -> 23 x 5 -> 21 x 3 -> 10 x 1; rows and columns are dropped
    "valid": dict(seed=806, blocks2d=((8, 3, 3, 2, dict(valid=True, pool_valid=True)), (8, 3, 3, 2, dict(valid=True, pool_valid=True))), edit=_lift()),
    # strided SAME convolutions.  s2x2: 2 x 3 filter -- total padding 1 along H (above 0, below 1), 2 along W.  s1x3: 3 x 2 filter, 13 -> 5 columns, total
    # padding 1 along W, 2 along H.  s2x1: the VALID strided case (49 -> 24 rows, 13 -> 11 columns)
    "s2x2": dict(seed=807, blocks2d=((8, 2, 3, 1, dict(stride=(2, 2))), (8, 3, 3, 2)), edit=_lift()),
    "s2x1": dict(seed=808, blocks2d=((8, 3, 3, 1, dict(stride=(2, 1), valid=True)), (8, 3, 3, 2)), edit=_lift()),
    "s1x3": dict(seed=809, blocks2d=((8, 3, 2, 1, dict(stride=(1, 3))), (8, 3, 3, 2)), edit=_lift()),
    # window != stride; pooling along one axis only
    "pool3s2": dict(seed=810, blocks2d=((8, 3, 3, 1, dict(pool=(3, 3), pool_stride=(2, 2))), (8, 3, 3, 2)), edit=_lift()),
    "pool2x1": dict(seed=811, blocks2d=((8, 3, 3, 1, dict(pool=(2, 1))), (8, 3, 3, 2)), edit=_lift()),
    "pool1x2": dict(seed=812, blocks2d=((8, 3, 3, 1, dict(pool=(1, 2))), (8, 3, 3, 2)), edit=_lift()),
    # three un-pooled convolutions, in_c 1 -> 6 -> 5 -> 3: no channel count a multiple of 4, an odd hand-off (49 * 13 * 3 = 1911)
    "nopool_chain": dict(seed=813, blocks2d=((6, 3, 3, 1), (5, 3, 3, 1), (3, 3, 3, 1)), edit=_lift()),
    "c64": dict(seed=814, blocks2d=((8, 3, 3, 2), (64, 3, 3, 2)), edit=_lift()),
    "c1": dict(seed=815, blocks2d=((1, 3, 3, 1), (8, 3, 3, 2)), edit=_lift()),
    # fused activation 0, 2 (relu_n1_to_1, no bias tensor) and 3 (relu6) on successive blocks
    "acts": dict(seed=816, blocks2d=((8, 3, 3, 2, dict(act=0)), (8, 3, 3, 1, dict(act=2, bias=False)), (8, 3, 3, 2, dict(act=3))), edit=_lift()),
    "hidden": dict(seed=817, blocks2d=_EI, dense=((32, 1),), edit=_lift()),
    # 49 x 40 features: one 3 x 3 block, pooled 2 x 4 to 25 x 10 x 8 = 2000 inputs
    "w40": dict(seed=818, **_M40, blocks2d=((8, 3, 3, 1, dict(pool=(2, 4))),), edit=_lift()),
    # the MFE block at 98 x 40: the widest image per wave (the float twin's wave count per workgroup drops to 5)
    "mfe98": dict(seed=819, dsp_block="mfe", num_filters=40, low=300, high=0, frame_stride=0.01, blocks2d=((8, 3, 3, 1, dict(pool=(4, 4))), (8, 3, 3, 2)),
                  edit=_lift(mfe=True)),
    "per_tensor": dict(seed=820, blocks2d=_EI, edit=_lift(per_tensor=True)),
    # the input zero point at both ends of int8 (the padding value is the zero point), on twins of k5x3
    "in_zp_m128": dict(seed=802, blocks2d=_K5X3, edit=_lift(in_zp=-128)),
    "in_zp_127": dict(seed=802, blocks2d=_K5X3, edit=_lift(in_zp=127)),
}
for _spec in CONV2D_SPECS.values():
    _spec.setdefault("logit_std", 1.5)

# (out_h, out_w, out_c) of every block's pooled output, as the table above promises them (tests/test_conv2d_graphs_host.py reads the blobs' tensors)
GEOMETRY = {
    "ei_2d": [(25, 7, 8), (13, 4, 16)], "k5x3": [(25, 7, 8), (13, 4, 8)], "k3x5": [(25, 7, 8), (13, 4, 8)], "k1x1": [(25, 7, 8), (25, 7, 12)],
    "k7x7_w4": [(25, 7, 8), (13, 4, 8), (13, 4, 8)], "valid": [(23, 5, 8), (10, 1, 8)], "s2x2": [(25, 7, 8), (13, 4, 8)], "s2x1": [(24, 11, 8), (12, 6, 8)],
    "s1x3": [(49, 5, 8), (25, 3, 8)], "pool3s2": [(25, 7, 8), (13, 4, 8)], "pool2x1": [(25, 13, 8), (13, 7, 8)], "pool1x2": [(49, 7, 8), (25, 4, 8)],
    "nopool_chain": [(49, 13, 6), (49, 13, 5), (49, 13, 3)], "c64": [(25, 7, 8), (13, 4, 64)], "c1": [(49, 13, 1), (25, 7, 8)],
    "acts": [(25, 7, 8), (25, 7, 8), (13, 4, 8)], "hidden": [(25, 7, 8), (13, 4, 16)], "w40": [(25, 10, 8)], "mfe98": [(25, 10, 8), (13, 5, 8)],
    "per_tensor": [(25, 7, 8), (13, 4, 16)], "in_zp_m128": [(25, 7, 8), (13, 4, 8)], "in_zp_127": [(25, 7, 8), (13, 4, 8)],
}
E2E_SPECS = ("ei_2d", "mfe98")


@functools.lru_cache(maxsize=None)
def conv2d_blob(name):
    return synth_model_blob(**CONV2D_SPECS[name])


@functools.lru_cache(maxsize=None)
def conv2d_twin(name):
    return D.dequantize_model.dequantize(conv2d_blob(name))


def _is_mfe(name):
    return CONV2D_SPECS[name].get("dsp_block") == "mfe"


def _shape(name):
    tens, nodes, _, _, _ = D.eon_import.parse_blob(conv2d_blob(name))
    return tens[nodes[0]["out"][0]]["dims"][1:3]


@functools.lru_cache(maxsize=None)
def conv2d_features(name):
    """[N_STD][features] float32: 32 rows as the DSP block makes them (standardised random values; MFE: uniform in [0, 1]), 7 rows past both ends of the
    input quantisation's range -- all high, all low, random and regular mixtures of both over the image, one with values just past the ends; the reference's
    input quantisation does not saturate there, it wraps (ei_run_classifier.h:436-444), and so does the oracle's -- and one all-zero row"""
    rng = np.random.default_rng(INPUT_SEED)
    h, w = _shape(name)
    F = h * w
    x = np.zeros((N_STD, F), np.float32)
    x[:32] = rng.uniform(0.0, 1.0, (32, F)) if _is_mfe(name) else rng.standard_normal((32, F))
    x[32], x[33] = 100.0, -100.0
    x[34] = np.where(rng.integers(0, 2, F), 100.0, -100.0)
    x[35] = np.where((np.arange(F) // w + np.arange(F) % w) % 2, 100.0, -100.0)          # a checkerboard over the image
    x[36] = np.where(np.arange(F) % w < w // 2, 100.0, -100.0)                           # left half high, right half low
    x[37] = np.where(np.arange(F) // w < h // 2, -100.0, 100.0)                          # upper half low, lower half high
    x[38] = rng.choice(np.float32([-9.0, -7.0, 7.0, 9.0]), F)
    return np.ascontiguousarray(x)


@functools.lru_cache(maxsize=None)
def conv2d_float_rows(name):
    """[N_FLOAT][features] float32, for the float twins: rows with +-0, subnormals, FLT_MAX neighbours, and one row holding +inf and one NaN at border and
    interior positions of the image (corners, an edge, the middle)"""
    rng = np.random.default_rng(INPUT_SEED + 1)
    h, w = _shape(name)
    F = h * w
    base = (rng.uniform(0.0, 1.0, (N_FLOAT, F)) if _is_mfe(name) else rng.standard_normal((N_FLOAT, F))).astype(np.float32)
    x = base.copy()
    spots = [0, w - 1, (h - 1) * w, h * w - 1, (h // 2) * w, (h // 2) * w + w // 2, w // 2, 3 * w + 2]      # corners, edges, interior
    x[0] = 0.0
    x[0, ::3] = -0.0
    x[1] = np.where(np.arange(F) % 2, np.float32(-0.0), np.float32(0.0))
    x[2] = rng.choice(np.float32([1e-45, -1e-45, 1e-40, -3e-39, 1.17549435e-38, 0.0]), F)                  # subnormals and the smallest normal
    x[3, spots] = np.float32([1e-45, -1e-45, 1e-40, -1e-40, 5e-39, -5e-39, 1e-38, -1e-38])
    fmax = np.finfo(np.float32).max
    x[4, spots] = np.float32([fmax, -fmax, np.nextafter(fmax, np.float32(0)), -np.nextafter(fmax, np.float32(0)), fmax, fmax, -fmax, fmax / 2])
    x[5, spots[:4]] = np.float32([fmax, -fmax, fmax, -fmax])
    x[6, [spots[0], spots[5], spots[3]]] = np.inf
    x[7, [spots[1], spots[5], spots[2]]] = np.nan
    return np.ascontiguousarray(x)


def conv2d_twin_features(name):
    """every row the float twin is run on: conv2d_features, then conv2d_float_rows"""
    return np.ascontiguousarray(np.concatenate([conv2d_features(name), conv2d_float_rows(name)]))


def block_shapes(blob):
    """(h, w, c) of every conv block's (pooled) output, as the blob's tensors state it"""
    tens, nodes, _, _, _ = D.eon_import.parse_blob(blob)
    out = []
    for k, nd in enumerate(nodes):
        if nd["op"] == 1:
            tid = nd["out"][0]
            if k + 1 < len(nodes) and nodes[k + 1]["op"] == 3:
                tid = nodes[k + 1]["out"][0]
            out.append(tuple(tens[tid]["dims"][1:]))
    return out


def same_bits_nan_by_position(a, b):
    """NaN by position, every other value bit for bit"""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and bool(((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())


def check_not_vacuous(name, blob, taps, out_rows, f_rows):
    """over the N_STD inputs' 32 ordinary rows: at most half of every conv block output sits on a clamp bound and it takes >= 16 distinct values (8 for a
    single channel); over all rows the graph gives >= 8 distinct score rows, int8 and float, and more than one class wins; AssertionError otherwise"""
    bounds = S.block_clamp_bounds(blob)
    tens, nodes, _, _, _ = D.eon_import.parse_blob(blob)
    for tid, (lo, hi) in bounds.items():
        v = taps[tid][:32]
        need = 8 if tens[tid]["dims"][-1] == 1 or v.shape[1] < 64 else 16
        assert len(np.unique(v)) >= need, "%s: block output %d takes %d values" % (name, tid, len(np.unique(v)))
        assert np.mean((v <= lo) | (v >= hi)) <= 0.5, "%s: %.2f of block output %d sits on a clamp bound" % (name, np.mean((v <= lo) | (v >= hi)), tid)
    assert len(np.unique(out_rows, axis=0)) >= 8 and len(np.unique(f_rows[:N_STD], axis=0)) >= 8, "%s: fewer than 8 distinct score rows" % name
    assert len(np.unique(np.argmax(out_rows, axis=1))) > 1 and len(np.unique(np.argmax(f_rows[:N_STD], axis=1))) > 1, "%s: one class wins every input" % name


def tensor_ids(blob):
    """ids of the tensors the fixture and the GPU test look at: every block output, the hidden tensors, the logits"""
    _, _, hidden, last, _, _ = D.graph_layout(blob)
    return D.block_outputs(blob) + hidden + [last]


def canonical_nan(a):
    """a float32 array with every NaN replaced by the one quiet NaN pattern (a digest then compares NaNs by position)"""
    a = np.ascontiguousarray(a, np.float32).copy()
    a[np.isnan(a)] = np.float32(np.nan)
    return a


# ---- refusals: name -> (spec, which twins: "both" / "int8" / "f32", what kws_last_error must say) -------------------------------------

def _conv(n, k=0):
    return [nd for nd in n if nd["op"] == 1][k]


def _edit_depthwise(t, n):
    _conv(n, 1)["op"] = 6


def _edit_add(t, n):
    """a per-channel ADD (int8 constant, ReLU) between the first convolution and its pool"""
    cv = _conv(n)
    y = t[cv["out"][0]]
    oc = y["dims"][-1]
    t.append(dict(type=9, dims=[oc], nbytes=oc, const=True, scale=[0.01], zero=[0], qdim=0, data=bytes(range(oc))))
    t.append(dict(y, dims=list(y["dims"]), scale=list(y["scale"]), zero=list(y["zero"])))
    idx = n.index(cv)
    n[idx + 1]["in"][0] = len(t) - 1
    n.insert(idx + 1, {"op": 2, "in": [cv["out"][0], len(t) - 2], "out": [len(t) - 1], "p": [1, 0, 0, 0, 0, 0, 0, 0], "beta": 0.0})


def _edit_dilation(t, n):
    _conv(n)["p"][5] = 2


def _edit_out_dims(t, n):
    y = t[_conv(n)["out"][0]]
    y["dims"][1] = 48
    y["nbytes"] = int(np.prod(y["dims"]))


def _edit_left_shift(t, n):
    _lift()(t, n)
    cv = _conv(n)
    for tid in (cv["out"][0], n[n.index(cv) + 1]["out"][0]):              # the convolution's output and its pool's: a scale so small the multiplier is 2^20
        t[tid]["scale"] = [float(np.float32(t[cv["in"][0]]["scale"][0] * t[cv["in"][1]]["scale"][0] / 2.0 ** 20))]


def _edit_pool_act(t, n):
    [nd for nd in n if nd["op"] == 3][0]["p"][5] = 1


_R = dict(seed=850)                  # (as drawn: a refused graph runs nowhere, so nothing is calibrated)
REFUSED = {
    "depthwise": (dict(_R, blocks2d=_EI, edit=_edit_depthwise), "both", "DEPTHWISE_CONV_2D"),
    "add": (dict(_R, blocks2d=_EI, edit=_edit_add), "both", "ADD"),
    "dilation": (dict(_R, blocks2d=_EI, edit=_edit_dilation), "both", "dilation 2 x 1"),
    "filter_9x3": (dict(_R, blocks2d=((8, 9, 3, 2), (8, 3, 3, 2))), "both", "filter sides 1 .. 7"),
    "stride_5": (dict(_R, blocks2d=((8, 3, 3, 1, dict(stride=(5, 1))), (8, 3, 3, 2))), "both", "stride 5 x 1"),
    "pool_8": (dict(_R, blocks2d=((8, 3, 3, 1, dict(pool=(8, 2))), (8, 3, 3, 1))), "both", "window 8 x 2"),
    "out_dims": (dict(_R, blocks2d=_EI, edit=_edit_out_dims), "both", "output shape"),
    # 98 x 40 x 64 un-pooled into a second block: a 100 x 42 x 64 image per wave
    "lds": (dict(_R, dsp_block="mfe", num_filters=40, low=300, high=0, frame_stride=0.01, blocks2d=((64, 3, 3, 1), (8, 3, 3, 1, dict(pool=(7, 7))))), "both", "LDS"),
    "left_shift": (dict(_R, blocks2d=_EI, edit=_edit_left_shift), "int8", "shifts left"),
    "pool_activation": (dict(_R, blocks2d=_EI, edit=_edit_pool_act), "int8", "fused activation 1"),
    # 49 x 40 features behind ONE 16-channel block pooled 2 x 2 flatten to 25 * 20 * 16 = 8000 values: past the dense stack's 4096 inputs (the stock graph's
    # two pools bring 49 x 40 down to 13 * 10 * 16 = 2080, which is served)
    "flatten_8000": (dict(_R, **_M40, blocks2d=((16, 3, 3, 2),)), "both", "4096 inputs"),
    "non_finite": (dict(_R, blocks2d=_EI), "f32", "non-finite"),
}


@functools.lru_cache(maxsize=None)
def refused_blobs():
    """{key: blob}: every REFUSED graph as the twins its entry names ("_f32": the float twin)"""
    out = {}
    for key, (spec, which, _) in REFUSED.items():
        blob = synth_model_blob(**spec)
        if which in ("both", "int8"):
            out[key] = blob
        if which in ("both", "f32"):
            twin = D.dequantize_model.dequantize(blob)
            if key == "non_finite":                      # one +inf in the second convolution's filter
                tens, nodes, t_in, t_out, meta = D.eon_import.parse_blob(twin)
                tw = tens[_conv(nodes, 1)["in"][1]]
                w = np.frombuffer(tw["data"], np.float32).copy()
                w[5] = np.inf
                tw["data"] = w.tobytes()
                twin = D.eon_import.serialise(tens, nodes, t_in, t_out, meta)
            out[key + "_f32"] = twin
    return out
