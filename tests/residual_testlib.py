"""Named residual graphs (CONV_2D and ADD(tensor, tensor) steps, each with an optional MAX_POOL_2D, in front of a dense stack) shared by
tests/test_residual_graphs_host.py, tests/test_gpu_residual_graphs.py, tools/make_golden_residual.py and tools/gpu_residual_rate.py: each an int8 graph
(tools/synth_model.py residual=, calibrated) and its float32 twin (tools/dequantize_model.py).  49 x 13 features and the shipped DSP block, 4 labels.  The
shapes are the smallest at which each mechanism can go wrong."""
import functools
import os

import numpy as np

import dense_testlib as D
from kws_testlib import GOLDEN, synth_model_blob

GOLDEN_RESIDUAL = os.path.join(GOLDEN, "residual_graphs.npz")
N_STD = 40               # rows every graph and twin is run on: 32 standardised random rows, 7 past both ends of the input quantisation, one all-zero row
N_FLOAT = 8              # rows of the float twins alone: signed zeros, subnormals, FLT_MAX neighbours, +inf, NaN
INPUT_SEED = 7171
H, W = 49, 13            # the feature matrix


def _c(name, src, oc, k, s=1, act=1, valid=False, lift=None):
    """a 1 x k convolution along time, stride s"""
    return (name, "conv", src, oc, 1, k, (1, s), valid, act) + (() if lift is None else (lift,))


def _c2(name, src, oc, kh, kw, s=(1, 1), act=1, valid=False):
    return (name, "conv", src, oc, kh, kw, s, valid, act)


def _identity(c=16):
    return (_c("c0", "in", c, 3), _c("m1", "c0", c, 9), _c("m2", "m1", c, 9, act=0), ("sum", "add", "c0", "m2", 1))


def _proj(src, i, oc, first=False):
    """a stride-2 block: main path 9-tap stride 2 + 9-tap, shortcut 1 x 1 stride 2 (relu), ADD relu; first: the shortcut listed before the main path"""
    main = (_c("m%da" % i, src, oc, 9, s=2), _c("m%db" % i, "m%da" % i, oc, 9, act=0))
    sc = (_c("s%d" % i, src, oc, 1, s=2),)
    add = (("b%d" % i, "add", "s%d" % i, "m%db" % i, 1),) if first else (("b%d" % i, "add", "m%db" % i, "s%d" % i, 1),)
    return (sc + main if first else main + sc) + add


_TC_PROJ = (_c("c0", "in", 16, 3, act=0),) + _proj("c0", 1, 24)
_TC_RES8 = (_c("c0", "in", 16, 3, act=0),) + _proj("c0", 1, 24) + _proj("b1", 2, 32) + _proj("b2", 3, 48)
_ID_CHAIN2 = (_c("c0", "in", 8, 3), _c("m1", "c0", 8, 3), _c("m2", "m1", 8, 3, act=0), ("a1", "add", "c0", "m2", 1),
              _c("n1", "a1", 8, 3), _c("n2", "n1", 8, 3, act=0), ("a2", "add", "a1", "n2", 3))


def _narrow(t, n):
    """the ADD's output scale at a quarter of its calibrated one: both int8 ends clamp.  Set last (a calibration pass would settle the range again); the
    tensors that rename the ADD's output and the bias scale of the layer that reads it follow"""
    ad = [nd for nd in n if nd["op"] == 2][-1]
    s = float(np.float32(t[ad["out"][0]]["scale"][0] * 0.25))
    _set_scale_downstream(t, n, ad["out"][0], s)


def _set_scale_downstream(t, n, tid, s, zero=None):
    ids = {tid}
    for nd in n:
        if nd["op"] in (0, 3) and nd["in"][0] in ids:
            ids.add(nd["out"][0])
    for i in ids:
        t[i]["scale"] = [s]
        if zero is not None:
            t[i]["zero"] = [zero]
    for nd in n:                                         # the int32 bias of a layer that reads it: the same real values at the new scale
        if nd["op"] in (1, 4) and nd["in"][0] in ids and len(nd["in"]) > 2 and nd["in"][2] >= 0:
            tb = t[nd["in"][2]]
            real = np.frombuffer(tb["data"], np.int32).astype(np.float64) * np.float64(tb["scale"])
            tb["scale"] = [float(np.float32(s) * np.float32(w_)) for w_ in t[nd["in"][1]]["scale"]]
            tb["data"] = np.clip(np.round(real / np.float64(tb["scale"])), -2.0 ** 31, 2.0 ** 31 - 1).astype(np.int32).tobytes()


def _all_pairs(ratio, out_k, out_zp, act):
    """ADD(input, input rotated by one channel) over every int8 operand pair: the 1 x 1 convolution's weights are 64 where ic == (oc + 1) % 13, its weight
    scale s2 / (64 s_in), zero bias, equal zero points -- a real multiplier of exactly 2^-6 on multiples of 64: it copies the bytes."""
    sm = D.synth_model

    def edit(t, n):
        cv = [nd for nd in n if nd["op"] == 1][0]
        ad = [nd for nd in n if nd["op"] == 2][0]
        tin = t[cv["in"][0]]
        s_in, z = tin["scale"][0], tin["zero"][0]
        s2 = float(np.float32(s_in * ratio))
        w = np.zeros((13, 1, 1, 13), np.int8)
        for oc in range(13):
            w[oc, 0, 0, (oc + 1) % 13] = 64
        tw, tb = t[cv["in"][1]], t[cv["in"][2]]
        tw["data"], tw["scale"], tw["zero"] = w.tobytes(), [float(np.float32(s2 / (64.0 * s_in)))], [0]
        tb["data"], tb["scale"], tb["zero"] = bytes(13 * 4), [float(np.float32(s_in) * np.float32(tw["scale"][0]))], [0]
        fc = [nd for nd in n if nd["op"] == 4][-1]
        sm.calibrate_head(t, n, 0, fc["in"][1], fc["in"][2], fc["out"][0], 1.5, 0, x=np.random.default_rng(5).standard_normal((256, H * W)))
        t[cv["out"][0]]["scale"], t[cv["out"][0]]["zero"] = [s2], [z]
        ad["p"][0] = act
        _set_scale_downstream(t, n, ad["out"][0], float(np.float32((s_in + s2) * out_k)), out_zp)
    return edit


def _all_pairs_steps(act):
    return (("rot", "conv", "in", 13, 1, 1, (1, 1), False, 0), ("sum", "add", "in", "rot", act))


RES_SPECS = {
    # identity shortcut: c0 feeds a 9-tap SAME convolution (margin 4) and the ADD (margin 0)
    "tc_identity": dict(seed=901, residual=_identity()),
    # projection shortcut: c0 feeds a 9-tap stride-2 convolution and a 1 x 1 stride-2 one; 49 -> 25 rows (total padding 8 and 0: odd split never, but SAME at
    # stride 2 over 49 rows pads 4 + 4 for the 9 taps and nothing for the 1 x 1)
    "tc_proj_s2": dict(seed=902, residual=_TC_PROJ),
    # three such blocks, 16 -> 24 -> 32 -> 48 channels, 49 -> 25 -> 13 -> 7 rows: 13 steps, hand-off 7 * 48 = 336
    "tc_res8": dict(seed=903, residual=_TC_RES8),
    # two chained identity blocks: the second skip is the first ADD's output; second ADD relu6
    "id_chain2": dict(seed=904, residual=_ID_CHAIN2),
    # the staged input with two consumers: conv 13 x (1 x 3) + the reshaped input, no activation
    "input_skip": dict(seed=905, residual=(_c("c0", "in", 13, 3, act=0), ("sum", "add", "c0", "in", 0))),
    # the same tensor twice; an even filter; relu_n1_to_1
    "add_self": dict(seed=906, residual=(_c("c0", "in", 5, 2, act=2), ("sum", "add", "c0", "c0", 2))),
    # node order and operand order: the shortcut listed first, ADD(shortcut, main)
    "shortcut_first": dict(seed=907, residual=(_c("c0", "in", 16, 3, act=0),) + _proj("c0", 1, 24, first=True)),
    # pooling ADD results: VALID conv (47 rows) -> conv -> ADD relu -> pool 3 stride 2 SAME (24 rows, the last window ragged)
    "add_pool_same": dict(seed=908, residual=(_c("c0", "in", 8, 3, valid=True), _c("m1", "c0", 8, 3, act=0), ("sum", "add", "c0", "m1", 1),
                                              ("p", "pool", "sum", (1, 3), (1, 2), False))),
    # tc_identity + MAX_POOL through the [1][W][1][C] renaming (window 2 stride 2 SAME: 25 rows, ragged)
    "tc_pool_keras": dict(seed=909, residual=_identity() + (("p", "pool", "sum", (1, 2), (1, 2), False, True),)),
    # both clamps busy: the ADD (no activation) writes at a quarter of its range's scale
    "narrow_out": dict(seed=910, residual=_identity()[:3] + (("sum", "add", "c0", "m2", 0),), edit=_narrow),
    # one channel, stride 4 (13 columns): one lane-item per position, narrow images
    "oc1": dict(seed=911, residual=(_c("c0", "in", 1, 3, s=4), _c("m1", "c0", 1, 3, act=0), ("sum", "add", "c0", "m1", 1))),
    "per_tensor": dict(seed=912, residual=_TC_PROJ, residual_opts=dict(per_tensor=True)),
    # operand zero points -128 (a ReLU output) and 127 (a convolution whose outputs are all negative: bias 6 deviations below zero)
    "zp_edges": dict(seed=913, residual=(_c("c0", "in", 8, 3), _c("m1", "c0", 8, 3, act=0, lift=-6.0), ("sum", "add", "c0", "m1", 0))),
    # four live tensors: while m3 is written, c0 and m1 (two skips) and m2 (its input) are live
    "slots4": dict(seed=914, residual=(_c("c0", "in", 8, 3), _c("m1", "c0", 8, 3), _c("m2", "m1", 8, 3), _c("m3", "m2", 8, 3, act=0),
                                       ("a1", "add", "m1", "m3", 1), ("a2", "add", "c0", "a1", 1))),
    "hidden": dict(seed=915, residual=_identity(), dense=((32, 1),)),
    # 2-D: conv 8 x 3 x 3 relu, pool 2 -> conv, conv -> ADD relu -> pool 2: 13 x 4 x 8 = 416
    "res2d_identity": dict(seed=916, two_d=True, residual=(_c2("c0", "in", 8, 3, 3), ("p0", "pool", "c0", (2, 2), (2, 2), False), _c2("m1", "p0", 8, 3, 3),
                                                           _c2("m2", "m1", 8, 3, 3, act=0), ("sum", "add", "p0", "m2", 1), ("p1", "pool", "sum", (2, 2), (2, 2), False))),
    # 2-D: main 16 x 3 x 3 stride 2 x 2 + conv; shortcut 1 x 1 stride 2 x 2; ADD relu; pool 3 x 2 VALID: 8 x 3 x 16 = 384
    "res2d_proj_s2": dict(seed=917, two_d=True, residual=(_c2("m1", "in", 16, 3, 3, s=(2, 2)), _c2("m2", "m1", 16, 3, 3, act=0),
                                                          _c2("sc", "in", 16, 1, 1, s=(2, 2)), ("sum", "add", "m2", "sc", 1),
                                                          ("p", "pool", "sum", (3, 2), (3, 2), True))),
    # every int8 operand pair through the ADD, at three operand-scale ratios
    "all_pairs_a": dict(seed=918, residual=_all_pairs_steps(0), edit=_all_pairs(1.0, 1.0, -5, 0)),
    "all_pairs_b": dict(seed=919, residual=_all_pairs_steps(1), edit=_all_pairs(16.0, 0.6, -128, 1)),
    "all_pairs_c": dict(seed=920, residual=_all_pairs_steps(3), edit=_all_pairs(1.0 / 3.7, 1.5, 40, 3)),
}

# (h, w, c) of every step's (pooled) output, as the table above promises them; the number of tensor + tensor ADDs
GEOMETRY = {
    "tc_identity": [(1, 49, 16)] * 4, "tc_proj_s2": [(1, 49, 16), (1, 25, 24), (1, 25, 24), (1, 25, 24), (1, 25, 24)],
    "tc_res8": [(1, 49, 16)] + [(1, 25, 24)] * 4 + [(1, 13, 32)] * 4 + [(1, 7, 48)] * 4,
    "id_chain2": [(1, 49, 8)] * 7, "input_skip": [(1, 49, 13)] * 2, "add_self": [(1, 49, 5)] * 2,
    "shortcut_first": [(1, 49, 16), (1, 25, 24), (1, 25, 24), (1, 25, 24), (1, 25, 24)],
    "add_pool_same": [(1, 47, 8), (1, 47, 8), (1, 24, 8)], "tc_pool_keras": [(1, 49, 16)] * 3 + [(25, 1, 16)], "narrow_out": [(1, 49, 16)] * 4,
    "oc1": [(1, 13, 1)] * 3, "per_tensor": [(1, 49, 16), (1, 25, 24), (1, 25, 24), (1, 25, 24), (1, 25, 24)], "zp_edges": [(1, 49, 8)] * 3,
    "slots4": [(1, 49, 8)] * 6, "hidden": [(1, 49, 16)] * 4, "res2d_identity": [(25, 7, 8), (25, 7, 8), (25, 7, 8), (13, 4, 8)],
    "res2d_proj_s2": [(25, 7, 16), (25, 7, 16), (25, 7, 16), (8, 3, 16)],
    "all_pairs_a": [(1, 49, 13)] * 2, "all_pairs_b": [(1, 49, 13)] * 2, "all_pairs_c": [(1, 49, 13)] * 2,
}
N_ADDS = {name: sum(1 for st in spec["residual"] if st[1] == "add") for name, spec in RES_SPECS.items()}
ALL_PAIRS = ("all_pairs_a", "all_pairs_b", "all_pairs_c")
BOUND_SHARE_EXEMPT = ("narrow_out",) + ALL_PAIRS
MULTI_CLIP_SPECS = ("tc_res8", "res2d_proj_s2")
E2E_SPECS = ("tc_res8", "res2d_identity")


@functools.lru_cache(maxsize=None)
def res_blob(name):
    return synth_model_blob(**RES_SPECS[name])


@functools.lru_cache(maxsize=None)
def res_twin(name):
    return D.dequantize_model.dequantize(res_blob(name))


@functools.lru_cache(maxsize=None)
def res_features(name=None):
    """[N_STD][features] float32: 32 standardised random rows (what cmvnw hands the network), 7 rows past both ends of the input quantisation's range (the
    reference's input quantisation wraps there, ei_run_classifier.h:436-444, and so does the oracle's), one all-zero row.  The same for every graph."""
    rng = np.random.default_rng(INPUT_SEED)
    F = H * W
    x = np.zeros((N_STD, F), np.float32)
    x[:32] = rng.standard_normal((32, F))
    x[32], x[33] = 100.0, -100.0
    x[34] = np.where(rng.integers(0, 2, F), 100.0, -100.0)
    x[35] = np.where((np.arange(F) // W + np.arange(F) % W) % 2, 100.0, -100.0)
    x[36] = np.where(np.arange(F) % W < W // 2, 100.0, -100.0)
    x[37] = np.where(np.arange(F) // W < H // 2, -100.0, 100.0)
    x[38] = rng.choice(np.float32([-9.0, -7.0, 7.0, 9.0]), F)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def res_float_rows(name=None):
    """[N_FLOAT][features] float32, for the float twins: rows with +-0, subnormals, FLT_MAX neighbours (their sums overflow: inf + (-inf) further on), and
    one row holding +inf and one NaN at border and interior positions of the matrix"""
    rng = np.random.default_rng(INPUT_SEED + 1)
    F = H * W
    x = rng.standard_normal((N_FLOAT, F)).astype(np.float32)
    spots = [0, W - 1, (H - 1) * W, H * W - 1, (H // 2) * W, (H // 2) * W + W // 2, W // 2, 3 * W + 2]
    x[0] = 0.0
    x[0, ::3] = -0.0
    x[1] = np.where(np.arange(F) % 2, np.float32(-0.0), np.float32(0.0))
    x[2] = rng.choice(np.float32([1e-45, -1e-45, 1e-40, -3e-39, 1.17549435e-38, 0.0]), F)
    x[3, spots] = np.float32([1e-45, -1e-45, 1e-40, -1e-40, 5e-39, -5e-39, 1e-38, -1e-38])
    fmax = np.finfo(np.float32).max
    x[4, spots] = np.float32([fmax, -fmax, np.nextafter(fmax, np.float32(0)), -np.nextafter(fmax, np.float32(0)), fmax, fmax, -fmax, fmax / 2])
    x[5, spots[:4]] = np.float32([fmax, -fmax, fmax, -fmax])
    x[6, [spots[0], spots[5], spots[3]]] = np.inf
    x[7, [spots[1], spots[5], spots[2]]] = np.nan
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def res_twin_features(name=None):
    """every row the float twin is run on: res_features, then res_float_rows"""
    x = np.ascontiguousarray(np.concatenate([res_features(), res_float_rows()]))
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def all_pairs_rows():
    """[223][637] int8 input tensors: frame f of row r holds six operand pairs on channels (0, 1), (2, 3) .. (10, 11) -- the ADD of all_pairs_* sums channel c
    and channel c + 1 at channel c -- so that the 65 536 (a, b) pairs all occur; channel 12 and the tail are zero"""
    per_row = H * 6
    n = (65536 + per_row - 1) // per_row
    q = np.zeros((n, H, W), np.int8)
    p = np.arange(n * per_row) % 65536
    a, b = (p // 256 - 128).astype(np.int8), (p % 256 - 128).astype(np.int8)
    q[:, :, 0:12:2] = a.reshape(n, H, 6)
    q[:, :, 1:12:2] = b.reshape(n, H, 6)
    q = np.ascontiguousarray(q.reshape(n, H * W))
    q.setflags(write=False)
    return q


def step_outputs(blob):
    """ids of the tensors that hold each step's (pooled) output, in step order: a CONV_2D's / ADD's output, or the output of the MAX_POOL_2D that reads it
    (through RESHAPEs, which keep the bytes) -- the steps' share of kws_nn_batch_device's tap_pooled"""
    _, nodes, _, _, _ = D.eon_import.parse_blob(blob)
    root, steps = {}, []
    for nd in nodes:
        o, i0 = nd["out"][0], nd["in"][0]
        if nd["op"] in (1, 2):
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


def add_outputs(blob):
    """{tensor id: (lo, hi)} of every tensor + tensor ADD's output with the int8 values its fused activation clamps to"""
    tens, nodes, _, _, _ = D.eon_import.parse_blob(blob)
    out = {}
    for nd in nodes:
        if nd["op"] == 2 and not tens[nd["in"][0]]["const"] and not tens[nd["in"][1]]["const"]:
            o = nd["out"][0]
            sc, zp, lo, hi = tens[o]["scale"][0], tens[o]["zero"][0], -128, 127
            if nd["p"][0] == 1:
                lo = max(lo, zp)
            elif nd["p"][0] == 2:
                lo, hi = max(lo, zp + int(round(-1.0 / sc))), min(hi, zp + int(round(1.0 / sc)))
            elif nd["p"][0] == 3:
                lo, hi = max(lo, zp), min(hi, zp + int(round(6.0 / sc)))
            out[o] = (lo, hi)
    return out


def tensor_ids(blob):
    """ids of the tensors the fixture and the GPU test look at: every step output, the hidden tensors, the logits"""
    _, _, hidden, last, _, _ = D.graph_layout(blob)
    return step_outputs(blob) + hidden + [last]


def watched_ids(blob):
    """tensor_ids plus the un-pooled ADD outputs (the non-vacuity conditions look at those)"""
    return sorted(set(tensor_ids(blob)) | set(add_outputs(blob)))


def oracle_int8(oracle, blob, feats=None, q=None):
    """the oracle's network on each feature row (or on the int8 input tensors q): (q [n][F], {tensor id: [n][size] int8} for watched_ids, out_q [n][labels],
    scores [n][labels])"""
    m = D.oracle_model(oracle, blob)
    if q is None:
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


def same_bits_nan_by_position(a, b):
    """NaN by position, every other value bit for bit"""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and bool(((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())


def canonical_nan(a):
    a = np.ascontiguousarray(a, np.float32).copy()
    a[np.isnan(a)] = np.float32(np.nan)
    return a


def check_not_vacuous(name, blob, taps, out_rows, f_rows):
    """conditions, not measurements: over the N_STD rows every tensor + tensor ADD output takes >= 24 distinct values and at most 0.6 of its entries sit on
    a clamp bound (BOUND_SHARE_EXEMPT: narrow_out, whose point is the clamps, and all_pairs_*, which run on their own rows); the graph gives >= 8 distinct
    score rows, int8 and float; AssertionError otherwise"""
    for tid, (lo, hi) in add_outputs(blob).items():
        v = taps[tid]
        assert len(np.unique(v)) >= 24, "%s: ADD output %d takes %d values" % (name, tid, len(np.unique(v)))
        share = float(np.mean((v <= lo) | (v >= hi)))
        assert name in BOUND_SHARE_EXEMPT or share <= 0.6, "%s: %.2f of ADD output %d sits on a clamp bound" % (name, share, tid)
    assert len(np.unique(out_rows, axis=0)) >= 8 and len(np.unique(f_rows[:N_STD], axis=0)) >= 8, "%s: fewer than 8 distinct score rows" % name


# ---- refusals: name -> (spec, which twins: "both" / "int8", what kws_last_error must say) -------------------------------------------

def _nodes(n, op):
    return [nd for nd in n if nd["op"] == op]


def _edit_broadcast(t, n):
    _nodes(n, 2)[0]["in"][1] = n[0]["out"][0]              # ADD(c0 [1][1][49][16], the reshaped input [1][1][49][13])


def _edit_const_operand(t, n):
    ad = _nodes(n, 2)[1]                                   # id_chain2's second ADD reads a constant; the first keeps the graph residual
    y = t[ad["out"][0]]
    size = int(np.prod(y["dims"]))
    t.append(dict(type=9, dims=list(y["dims"]), nbytes=size, const=True, scale=[0.01], zero=[0], qdim=0, data=bytes(size)))
    ad["in"][1] = len(t) - 1


def _edit_depthwise(t, n):
    _nodes(n, 1)[1]["op"] = 6


def _edit_dilation(t, n):
    _nodes(n, 1)[1]["p"][4] = 2


def _edit_add_multiplier(t, n):
    ad = _nodes(n, 2)[0]
    s = 2.0 * max(t[ad["in"][0]]["scale"][0], t[ad["in"][1]]["scale"][0]) / 2.0 ** 20 / 2.0          # the output multiplier becomes 2
    _set_scale_downstream(t, n, ad["out"][0], float(np.float32(s)))


def _edit_out_dims(t, n):
    y = t[_nodes(n, 1)[1]["out"][0]]
    y["dims"][2] = 48
    y["nbytes"] = int(np.prod(y["dims"]))


def _edit_pool_act(t, n):
    _nodes(n, 3)[0]["p"][5] = 1


def _chain(blocks):
    st = [_c("c0", "in", 4, 3)]
    prev = "c0"
    for k in range(blocks):
        st += [_c("m%d" % k, prev, 4, 3, act=0), ("a%d" % k, "add", prev, "m%d" % k, 1)]
        prev = "a%d" % k
    return tuple(st)


_R = dict(seed=950)
_MFE98 = dict(dsp_block="mfe", num_filters=40, low=300, high=0, frame_stride=0.01, calib=np.random.default_rng(3).uniform(0.0, 1.0, (4, 98 * 40)))
REFUSED = {
    "broadcast": (dict(_R, residual=_identity(), edit=_edit_broadcast), "both", "broadcasting"),
    "const_operand": (dict(_R, residual=_ID_CHAIN2, edit=_edit_const_operand), "both", "constant operand"),
    "depthwise": (dict(_R, residual=_identity(), edit=_edit_depthwise), "both", "DEPTHWISE_CONV_2D"),
    "dilation": (dict(_R, residual=_identity(), edit=_edit_dilation), "both", "dilation 1 x 2"),
    "steps_17": (dict(_R, residual=_chain(8)), "both", "more than 16 steps"),
    # while m4 is written c0, m1, m2 (three skips) and m3 are live
    "live_5": (dict(_R, residual=(_c("c0", "in", 4, 3), _c("m1", "c0", 4, 3), _c("m2", "m1", 4, 3), _c("m3", "m2", 4, 3), _c("m4", "m3", 4, 3, act=0),
                                  ("a1", "add", "m2", "m4", 1), ("a2", "add", "m1", "a1", 1), ("a3", "add", "c0", "a2", 1))), "both", "5 tensors live"),
    # the ADD's output feeds an (identity) pool and a second ADD
    "shared_pool_input": (dict(_R, residual=(_c("c0", "in", 4, 3), ("a", "add", "c0", "c0", 1), ("p", "pool", "a", (1, 1), (1, 1), False),
                                             ("z", "add", "a", "p", 1))), "both", "shares its input"),
    "add_multiplier": (dict(_R, residual=_identity(), edit=_edit_add_multiplier), "int8", "output multiplier"),
    "out_dims": (dict(_R, residual=_identity(), edit=_edit_out_dims), "both", "output shape"),
    "pool_activation": (dict(_R, residual=RES_SPECS["add_pool_same"]["residual"], edit=_edit_pool_act), "int8", "fused activation 1"),
    # 98 x 40 x 64 images: 250 KB each
    "lds": (dict(_R, **_MFE98, two_d=True, residual=(_c2("c0", "in", 64, 3, 3), _c2("m1", "c0", 64, 3, 3, act=0), ("a", "add", "c0", "m1", 1),
                                                     ("p", "pool", "a", (7, 7), (7, 7), False), _c2("f", "p", 8, 1, 1))), "both", "LDS"),
}


@functools.lru_cache(maxsize=None)
def refused_blobs():
    """{key: blob}: every REFUSED graph as the twins its entry names ("_f32": the float twin)"""
    out = {}
    for key, (spec, which, _) in REFUSED.items():
        blob = synth_model_blob(**spec)
        out[key] = blob
        if which == "both":
            out[key + "_f32"] = D.dequantize_model.dequantize(blob)
    return out
