"""Named graphs with DEPTHWISE_CONV_2D steps on the step trunks (depthwise-separable 2-D graphs, and depthwise steps next to a skip connection)
shared by tests/test_dwres_graphs_host.py, tests/test_gpu_dwres_graphs.py, tools/make_golden_dwres.py and tools/gpu_dwres_rate.py: each an int8 graph
(tools/synth_model.py residual= with "dw" steps, calibrated) and its float32 twin (tools/dequantize_model.py).  49 x 13 features and the shipped DSP block,
4 labels; the graphs run on residual_testlib's input rows (40 + 8).  The shapes are the smallest at which each mechanism can go wrong."""
import functools
import os

import numpy as np

import dense_testlib as D
import residual_testlib as R
from kws_testlib import GOLDEN, synth_model_blob

GOLDEN_DWRES = os.path.join(GOLDEN, "dwres_graphs.npz")
N_STD, N_FLOAT, H, W = R.N_STD, R.N_FLOAT, R.H, R.W
res_features, res_twin_features = R.res_features, R.res_twin_features
same_bits_nan_by_position, canonical_nan = R.same_bits_nan_by_position, R.canonical_nan


def _c(name, src, oc, k, s=1, act=1, valid=False):
    """a 1 x k convolution along time, stride s"""
    return (name, "conv", src, oc, 1, k, (1, s), valid, act)


def _c2(name, src, oc, kh, kw, s=(1, 1), act=1, valid=False):
    return (name, "conv", src, oc, kh, kw, s, valid, act)


def _d(name, src, mult, k, s=1, act=0, valid=False):
    """a 1 x k depthwise convolution along time"""
    return (name, "dw", src, mult, 1, k, (1, s), valid, act)


def _d2(name, src, mult, kh, kw, s=(1, 1), act=1, valid=False):
    return (name, "dw", src, mult, kh, kw, s, valid, act)


def _pool(name, src, win, stride, valid=False):
    return (name, "pool", src, win, stride, valid)


def _edit_act_ignored(t, n):
    """the depthwise step's (ReLU) output tensor at zero point 0 and twice its scale: values below the zero point are representable, and the int8 kernel --
    which ignores the fused activation -- writes them; the bias of the layer that reads the tensor follows"""
    dw = [nd for nd in n if nd["op"] == 6][0]
    o = dw["out"][0]
    assert dw["p"][3] == 1
    R._set_scale_downstream(t, n, o, float(np.float32(t[o]["scale"][0] * 2.0)), 0)


_MBX = (_c("c0", "in", 16, 3), _d("d1", "c0", 1, 9), _c("p1", "d1", 16, 1), _d("d2", "p1", 1, 9), _c("p2", "d2", 16, 1, act=0), _c("sc", "c0", 16, 1, act=0),
        ("sum", "add", "p2", "sc", 1))
_MNV2 = (_c2("c0", "in", 8, 3, 3, s=(2, 2), act=3), _c2("e", "c0", 24, 1, 1, act=3), _d2("d", "e", 1, 3, 3, act=3), _c2("p", "d", 8, 1, 1, act=0),
         ("sum", "add", "c0", "p", 0))
_DS2D = (_c2("c0", "in", 8, 3, 3, s=(2, 1)), _d2("d", "c0", 1, 3, 3), _c2("p", "d", 16, 1, 1), _pool("q", "p", (2, 2), (2, 2)))
_SMALL = (_c2("c0", "in", 8, 3, 3, s=(2, 2)), _d2("d", "c0", 1, 3, 3), _c2("p", "d", 8, 1, 1))

DW_SPECS = {
    # 1-D, MatchboxNet-style: c0 feeds a 9-tap depthwise step (margin 4) and the 1 x 1 projection shortcut (margin 0)
    "mbx_block": dict(seed=1001, residual=_MBX),
    # 2-D inverted residual: expand 8 -> 24, depthwise 3 x 3, project 24 -> 8, identity skip; 25 x 7 images, hand-off 1400
    "mnv2_ir": dict(seed=1002, two_d=True, residual=_MNV2),
    # 2-D, NO ADD: the routing rule; 25 x 13 x 8 -> pool 2 x 2 (13 x 7 x 16 = 1456, the last windows ragged)
    "ds2d_plain": dict(seed=1003, two_d=True, residual=_DS2D),
    # depth multiplier 8 on the 1-channel input image (ic = 0 for every oc), stride 2 x 2, then a pointwise step
    "dw_in_m8": dict(seed=1004, two_d=True, residual=(_d2("d", "in", 8, 3, 3, s=(2, 2)), _c2("p", "d", 4, 1, 1))),
    # 1-D: multiplier 2 on the 13-channel input (26 channels: ic = oc / 2 on an odd channel count), ADD of the result with itself
    "dw_m2_13": dict(seed=1005, residual=(_d("d", "in", 2, 3, act=1), ("sum", "add", "d", "d", 1))),
    # an even 4 x 4 SAME filter: padding 1 before, 2 after
    "dw_k4_same": dict(seed=1006, two_d=True, residual=(_c2("c0", "in", 4, 3, 3, s=(2, 2)), _d2("d", "c0", 1, 4, 4), _c2("p", "d", 8, 1, 1))),
    # VALID conv (47 x 11), VALID depthwise 3 x 3 stride 2 x 2 (23 x 5) with a fused 2 x 2 SAME pool (12 x 3: the last window of both axes is clipped)
    "dw_s2_pool_ragged": dict(seed=1007, two_d=True, residual=(_c2("c0", "in", 8, 3, 3, valid=True), _d2("d", "c0", 1, 3, 3, s=(2, 2), valid=True),
                                                               _pool("q", "d", (2, 2), (2, 2)), _c2("p", "q", 8, 1, 1))),
    # a depthwise step is the last step: it writes the hand-off row
    "dw_last": dict(seed=1008, two_d=True, residual=_SMALL[:2]),
    # no bias tensor (and no activation: without a bias nothing lifts the pre-activations, a ReLU would park more than half of them)
    "dw_no_bias": dict(seed=1009, two_d=True, residual=(_SMALL[0], _d2("d", "c0", 1, 3, 3, act=0), _SMALL[2]), residual_opts=dict(no_bias=("d",))),
    "dw_per_tensor": dict(seed=1010, two_d=True, residual=_SMALL, residual_opts=dict(per_tensor=True)),
    "dw_act_ignored": dict(seed=1011, two_d=True, residual=_SMALL, edit=_edit_act_ignored),
    # 1-D: 64 channels and a 1 x 16 filter, both at their bounds; 25 rows, pooled to 13 (832 values)
    "dw_oc64_k16": dict(seed=1012, residual=(_c("c0", "in", 64, 3, s=2), _d("d", "c0", 1, 16), ("sum", "add", "c0", "d", 1), _pool("q", "sum", (1, 2), (1, 2)))),
}

# (h, w, c) of every step's (pooled) output; tensor + tensor ADDs; depthwise steps
GEOMETRY = {
    "mbx_block": [(1, 49, 16)] * 7, "mnv2_ir": [(25, 7, 8), (25, 7, 24), (25, 7, 24), (25, 7, 8), (25, 7, 8)],
    "ds2d_plain": [(25, 13, 8), (25, 13, 8), (13, 7, 16)], "dw_in_m8": [(25, 7, 8), (25, 7, 4)], "dw_m2_13": [(1, 49, 26)] * 2,
    "dw_k4_same": [(25, 7, 4), (25, 7, 4), (25, 7, 8)], "dw_s2_pool_ragged": [(47, 11, 8), (12, 3, 8), (12, 3, 8)], "dw_last": [(25, 7, 8)] * 2,
    "dw_no_bias": [(25, 7, 8)] * 3, "dw_per_tensor": [(25, 7, 8)] * 3, "dw_act_ignored": [(25, 7, 8)] * 3,
    "dw_oc64_k16": [(1, 25, 64), (1, 25, 64), (1, 13, 64)],
}
N_ADDS = {name: sum(1 for st in spec["residual"] if st[1] == "add") for name, spec in DW_SPECS.items()}
N_DW = {name: sum(1 for st in spec["residual"] if st[1] == "dw") for name, spec in DW_SPECS.items()}
MULTI_CLIP_SPECS = ("mbx_block", "mnv2_ir")
E2E_SPECS = ("ds2d_plain", "mnv2_ir")
# check_not_vacuous: a depthwise output without both int8 ends must have at least CLAMP_SHARE_MIN of its entries on one; none may have more than CLAMP_SHARE_MAX
CLAMP_SHARE_MIN, CLAMP_SHARE_MAX = 0.002, 0.6


@functools.lru_cache(maxsize=None)
def dw_blob(name):
    return synth_model_blob(**DW_SPECS[name])


@functools.lru_cache(maxsize=None)
def dw_twin(name):
    return D.dequantize_model.dequantize(dw_blob(name))


def conv_twin_spec(name):
    """the spec in which every depthwise step is a full CONV_2D of the same filter size, stride, padding and activation (tools/gpu_dwres_rate.py); with an
    ADD the step trunks serve it, without one it is a CONV_2D + MAX_POOL_2D chain of the 2-D family"""
    spec = dict(DW_SPECS[name])
    chans = {"in": 1 if spec.get("two_d") else W}
    steps = []
    for st in spec["residual"]:
        if st[1] == "dw":
            st = (st[0], "conv", st[2], chans[st[2]] * st[3]) + tuple(st[4:9])
        chans[st[0]] = st[3] if st[1] == "conv" else chans[st[2]]
        steps.append(st)
    spec["residual"] = tuple(steps)
    return spec


def step_outputs(blob):
    """ids of the tensors that hold each step's (pooled) output, in step order: a CONV_2D's / DEPTHWISE_CONV_2D's / ADD's output, or the output of the
    MAX_POOL_2D that reads it (through RESHAPEs, which keep the bytes) -- the steps' share of kws_nn_batch_device's tap_pooled"""
    _, nodes, _, _, _ = D.eon_import.parse_blob(blob)
    root, steps = {}, []
    for nd in nodes:
        o, i0 = nd["out"][0], nd["in"][0]
        if nd["op"] in (1, 2, 6):
            steps.append(o)
            root[o] = len(steps) - 1
        elif nd["op"] == 0 and i0 in root:
            root[o] = root[i0]
        elif nd["op"] == 3 and i0 in root:
            k = root[i0]
            root = {t: v for t, v in root.items() if v != k}
            steps[k] = o
            root[o] = k
    return steps


def dw_outputs(blob):
    """ids of every DEPTHWISE_CONV_2D's own (un-pooled) output tensor"""
    _, nodes, _, _, _ = D.eon_import.parse_blob(blob)
    return [nd["out"][0] for nd in nodes if nd["op"] == 6]


def tensor_ids(blob):
    """ids of the tensors the fixture and the GPU test look at: every step output, the hidden tensors, the logits"""
    _, _, hidden, last, _, _ = D.graph_layout(blob)
    return step_outputs(blob) + hidden + [last]


def watched_ids(blob):
    """tensor_ids plus the un-pooled depthwise outputs (the non-vacuity conditions look at those)"""
    return sorted(set(tensor_ids(blob)) | set(dw_outputs(blob)))


def oracle_int8(oracle, blob, feats):
    """the oracle's network on each feature row: (q [n][F], {tensor id: [n][size] int8} for watched_ids, out_q [n][labels], scores [n][labels])"""
    m = D.oracle_model(oracle, blob)
    q = np.stack([m.quantize_input(f) for f in feats])
    taps = {i: [] for i in watched_ids(blob)}
    outs = []
    for row in q:
        out, tp = m.nn_invoke(row, taps=True)
        outs.append(out)
        for i in taps:
            taps[i].append(tp[i].copy())
    outs = np.stack(outs)
    return q, {i: np.stack(v) for i, v in taps.items()}, outs, np.stack([m.dequantize(o) for o in outs])


def oracle_f32(oracle, twin, feats):
    """float twin: ({tensor id: [n][size] float32} for tensor_ids, scores [n][labels])"""
    m = D.oracle_model(oracle, twin)
    taps = {i: [] for i in tensor_ids(twin)}
    outs = []
    for row in feats:
        out, tp = m.nn_invoke_f32(row, taps=True)
        outs.append(out)
        for i in taps:
            taps[i].append(tp[i].copy())
    return {i: np.stack(v) for i, v in taps.items()}, np.stack(outs)


def check_not_vacuous(name, blob, taps, out_rows, f_rows):
    """conditions, not measurements: over the N_STD rows every depthwise step's output takes >= 24 distinct values and holds both int8 ends (-128 and 127:
    both sides of the int8 kernel's clamp are exercised) or, failing that, at least CLAMP_SHARE_MIN of its entries sit on an end; at most CLAMP_SHARE_MAX
    do; the graph gives >= 8 distinct score rows, int8 and float; AssertionError otherwise"""
    for tid in dw_outputs(blob):
        v = taps[tid]
        assert len(np.unique(v)) >= 24, "%s: depthwise output %d takes %d values" % (name, tid, len(np.unique(v)))
        both = bool((v == -128).any() and (v == 127).any())
        share = float(np.mean((v == -128) | (v == 127)))
        assert both or share >= CLAMP_SHARE_MIN, "%s: depthwise output %d: %.4f of it clamped, one end missing" % (name, tid, share)
        assert share <= CLAMP_SHARE_MAX, "%s: %.2f of depthwise output %d sits on an int8 end" % (name, share, tid)
    assert len(np.unique(out_rows, axis=0)) >= 8 and len(np.unique(f_rows[:N_STD], axis=0)) >= 8, "%s: fewer than 8 distinct score rows" % name


# ---- refusals: name -> (spec, which twins: "both" / "int8" / "f32", the words kws_last_error must contain) ---------------------------

def _dwn(n):
    return [nd for nd in n if nd["op"] == 6][0]


def _edit_filter_dims(t, n):
    w = t[_dwn(n)["in"][1]]                                # [1][3][3][8] -> [3][1][3][8]: the same bytes, the same channels
    w["dims"] = [3, 1, 3, 8]


def _edit_mult_zero(t, n):
    _dwn(n)["p"][6] = 0


def _edit_mult_disagrees(t, n):
    _dwn(n)["p"][6] = 2                                    # 8 channels in, 8 out: the tensors say 1


def _edit_dw_dilation(t, n):
    _dwn(n)["p"][4] = 2


def _edit_left_shift(t, n):
    """the depthwise step's output scale so small that its requantisation shifts left by more than its accumulators can bear"""
    o = _dwn(n)["out"][0]
    R._set_scale_downstream(t, n, o, float(np.float32(t[o]["scale"][0] * 2.0 ** -22)))


def _edit_non_finite(t, n):
    w = t[_dwn(n)["in"][1]]
    w["scale"][3] = float("inf")                           # the twin's weights of channel 3 are +-inf (and NaN where the int8 weight is 0)


_RF = dict(seed=1050, two_d=True)
REFUSED = {
    "filter_dims": (dict(_RF, residual=_SMALL, edit=_edit_filter_dims), "both", ("conv 2:", "DEPTHWISE_CONV_2D", "filter")),
    "mult_zero": (dict(_RF, residual=_SMALL, edit=_edit_mult_zero), "both", ("conv 2:", "DEPTHWISE_CONV_2D", "multiplier 0")),
    "mult_disagrees": (dict(_RF, residual=_SMALL, edit=_edit_mult_disagrees), "both", ("conv 2:", "DEPTHWISE_CONV_2D", "multiplier 2")),
    # 9 channels x multiplier 8 = 72 output channels
    "oc_72": (dict(_RF, residual=(_c2("c0", "in", 9, 3, 3, s=(2, 2)), _d2("d", "c0", 8, 3, 3, s=(2, 2)), _c2("p", "d", 8, 1, 1))), "both",
              ("conv 2:", "DEPTHWISE_CONV_2D", "at most 64")),
    "dilation": (dict(_RF, residual=_SMALL, edit=_edit_dw_dilation), "both", ("conv 2:", "DEPTHWISE_CONV_2D", "dilation 1 x 2")),
    "left_shift": (dict(_RF, residual=_SMALL, edit=_edit_left_shift), "int8", ("conv 2:", "DEPTHWISE_CONV_2D", "shifts left")),
    "non_finite": (dict(_RF, residual=_SMALL, edit=_edit_non_finite), "f32", ("conv 2:", "DEPTHWISE_CONV_2D", "non-finite")),
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
            out[key + "_f32"] = D.dequantize_model.dequantize(blob)
    return out
