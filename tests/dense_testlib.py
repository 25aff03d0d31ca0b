"""Named graphs with dense stacks shared by tests/test_dense_graphs_host.py, tests/test_gpu_dense.py and tools/make_golden_dense.py:
dense-only classifiers on the feature matrix and conv trunks with hidden FULLY_CONNECTED layers, each int8 with a float32 twin
(tools/dequantize_model.py).  DSP fields are the shipped l476_no_yes ones (tools/synth_model.py's defaults) unless a spec says otherwise, so
that the graphs can share a bank with it."""
import functools
import os
import sys
import tempfile

import numpy as np

from kws_testlib import GOLDEN, GraphEdit, OracleModel, ROOT, synth_model_blob

sys.path.insert(0, os.path.join(ROOT, "tools"))
import dequantize_model  # noqa: E402
import eon_import  # noqa: E402
import synth_model  # noqa: E402

GOLDEN_DENSE = os.path.join(GOLDEN, "dense_l476.npz")
N_INPUTS = 64            # inputs per model of the CPU pins and the fixture: the oracle's feature matrices of 56 synth clips + 8 uniform-random rows
N_SYNTH = 56
INPUT_SEED = 4242

UNIT_TAILS = (1, 15, 16, 17, 63, 64, 65, 255, 256)


@functools.lru_cache(maxsize=None)
def _shipped_features():
    """the oracle's feature matrices of 256 synth clips at the shipped DSP block (every d0_q_* graph's): what the edits calibrate on"""
    o = _get_oracle()
    m = oracle_model(o, synth_model_blob(**_H20))
    f = m.run_batch(o.synth(INPUT_SEED + 2, 0, 224), want_features=True)[1].astype(np.float64)
    # ... and uniform-random rows in the proportion of dense_features(): with half of the input range cut off (zero points of -128 / 127) a graph
    # answers their larger mean, and a range calibrated without them saturates
    return np.concatenate([f, np.random.default_rng(INPUT_SEED + 3).uniform(-3.0, 3.0, (32, f.shape[1]))])


def _recalibrate(t, n, t_in, hidden=True):
    """hidden biases, activation ranges and head again, on what the (edited) input quantisation lets through of real feature matrices"""
    x = _shipped_features()
    s, z = t[t_in]["scale"][0], t[t_in]["zero"][0]
    x = (np.clip(np.round(x / s) + z, -128, 127) - z) * s
    fcs = [nd for nd in n if nd["op"] == 4]
    if hidden:
        synth_model.calibrate_hidden(t, n, t_in, fcs[:-1], x)
    head = fcs[-1]
    synth_model.calibrate_head(t, n, t_in, head["in"][1], head["in"][2], head["out"][0], 1.5, 0, x=x)


def _fcs(n):
    return [nd for nd in n if nd["op"] == 4]


def _q_w_zp(v):
    def f(t, n):                                         # every dense layer's weight zero point (w_off * sum(x) per clip)
        for nd in _fcs(n):
            t[nd["in"][1]]["zero"] = [v]
        _recalibrate(t, n, 0)
    return f


def _q_in_zp(v):
    def f(t, n):
        # the second layer's input zero point at an end of int8: the first hidden tensor is all-negative without activation (its range ends at 0:
        # zero point 127) or all-positive under its ReLU (-128, and hardly an output on the bound)
        fcs = _fcs(n)
        x = _shipped_features()
        if v == 127:
            fcs[0]["p"][0] = 0
        synth_model.calibrate_hidden(t, n, 0, fcs[:1], x, lift=-4.0 if v == 127 else 3.0)
        synth_model.calibrate_hidden(t, n, 0, fcs[1:-1], x)
        _recalibrate(t, n, 0, hidden=False)
        GraphEdit(t, n).set_quant(fcs[0]["out"][0], zero=v)
    return f


def _q_mult(eff, pow2):
    def f(t, n):
        # the second hidden layer (K = 20) with a multiplier of 1 or more (a left shift): two +-1 weights per unit and small biases, as the
        # conv edges do it -- with drawn weights such a layer clamps nearly every output
        g = GraphEdit(t, n)
        nd = _fcs(n)[1]
        g.sparse_weights(nd)
        g.set_bias(nd, np.random.default_rng(5).integers(20, 90, 10))
        (g.set_multiplier_pow2 if pow2 else g.set_multiplier)(nd, eff)
        g.finish()
        # the head again, on the new hidden tensor
        _recalibrate(t, n, 0, hidden=False)
        # calibrate_head settles every activation range again: the edited layer keeps its multiplier only if it is set last
        (g.set_multiplier_pow2 if pow2 else g.set_multiplier)(nd, eff)
        g.finish()
    return f


def _q_no_bias(t, n):
    # hidden layers without a bias tensor; without their ReLU too: un-biased pre-activations are zero-mean, a ReLU would park half of them on its bound
    for nd in _fcs(n)[:-1]:
        nd["in"] = nd["in"][:2] + [-1]
        nd["p"][0] = 0
    _recalibrate(t, n, 0, hidden=False)


def _q_relu_n1(t, n):
    # ReLU_N1_TO_1 on the hidden layers: their weight scales are set so that the pre-activations' deviation is 0.4 around 0 (as drawn they are tens of
    # units wide and every output would sit on -1 or 1)
    x = _shipped_features()
    for nd in _fcs(n)[:-1]:
        nd["p"][0] = 2
        idx = n.index(nd)
        synth_model.calibrate_ranges(t, n[:idx], 0, x)
        a = synth_model.float_forward(t, n[:idx], 0, x)[nd["in"][0]]
        z = a.reshape(len(a), -1) @ synth_model.dequantised_constants(t)[nd["in"][1]].T
        tw = t[nd["in"][1]]
        tw["scale"] = [float(np.float32(tw["scale"][0] * 0.4 / z.std()))]
        synth_model.calibrate_hidden(t, n, 0, [nd], x, lift=0.0)
    _recalibrate(t, n, 0, hidden=False)


_H20 = dict(seed=301, blocks=(), dense=((20, 1), (10, 1)))
DENSE_SPECS = {
    "d0_logreg": dict(seed=300, blocks=(), logit_std=1.5),                                               # a single layer, K = 637 = 9 * 64 + 61
    "d0_h20_h10": dict(_H20),                                                                            # the stock dense classifier
    "c2_h64": dict(seed=302, dense=((64, 1),)),                                                          # the shipped trunk (head reads 10 values)
    "c1_h48_h16": dict(seed=303, blocks=((8, 3, 2),), dense=((48, 3), (16, 0)), n_labels=12),
    "d0_m40_h128": dict(seed=304, num_filters=40, ncep=40, low=300, high=0, blocks=(), dense=((128, 1),)),   # K = 30 * 64 + 40, eight unit tiles
    "d0_mfe_h32": dict(seed=305, dsp_block="mfe", num_filters=40, low=300, high=0, frame_stride=0.01, blocks=(), dense=((32, 1),)),   # 98 x 40
    # one un-pooled block of 64 channels: 49 x 64 = 3136 hand-off values per clip -- the trunk's 16 MiB hand-off buffer holds 5349 clips of the int8
    # graph and 1337 of the twin, so a batch of 5400 (EXTRA_BATCHES) walks more than one chunk in both
    "c1w_h32": dict(seed=307, blocks=((64, 3, 1),), dense=((32, 1),)),
    "d0_l48": dict(seed=306, blocks=(), dense=((32, 1),), n_labels=48),
    "d0_q_wzp_p5": dict(_H20, edit=_q_w_zp(5)),
    "d0_q_wzp_m5": dict(_H20, edit=_q_w_zp(-5)),
    "d0_q_inzp_m128": dict(_H20, edit=_q_in_zp(-128)),
    "d0_q_inzp_127": dict(_H20, edit=_q_in_zp(127)),
    "d0_q_mult_one": dict(_H20, edit=_q_mult(1.0, True)),
    "d0_q_mult_1_37": dict(_H20, edit=_q_mult(1.37, False)),
    "d0_q_no_bias": dict(_H20, edit=_q_no_bias),
    "d0_q_relu_n1": dict(_H20, edit=_q_relu_n1),
}
for _u in UNIT_TAILS:
    DENSE_SPECS["d0_u%d" % _u] = dict(seed=310 + _u, blocks=(), dense=((_u, 1),))

EXTRA_BATCHES = {"c1w_h32": (5400,)}

_oracle = None


def _get_oracle():
    global _oracle
    if _oracle is None:
        from kws_testlib import Oracle
        _oracle = Oracle()
    return _oracle


def oracle_model(oracle, blob):
    """OracleModel of a blob (it loads from a path)"""
    with tempfile.NamedTemporaryFile(suffix=".kwsm") as f:
        f.write(blob)
        f.flush()
        return OracleModel(oracle, f.name)


@functools.lru_cache(maxsize=None)
def dense_blob(name):
    spec = dict(DENSE_SPECS[name])
    if spec.get("dsp_block") == "mfe":
        # the MFE block's output is no standardised matrix: calibrate on the oracle's own feature matrices of synth clips
        o = _get_oracle()
        m = oracle_model(o, synth_model_blob(**spec))
        _, f, _ = m.run_batch(o.synth(INPUT_SEED + 1, 0, 64), want_features=True)
        spec["calib"] = f
    return synth_model_blob(**spec)


@functools.lru_cache(maxsize=None)
def dense_twin(name):
    return dequantize_model.dequantize(dense_blob(name))


@functools.lru_cache(maxsize=None)
def dense_features(name):
    """[N_INPUTS][features] float32: the oracle's feature matrices of synth clips, then uniform-random rows"""
    o = _get_oracle()
    m = oracle_model(o, dense_blob(name))
    _, f, _ = m.run_batch(o.synth(INPUT_SEED, 0, N_SYNTH), want_features=True)
    lo, hi = (0.0, 1.0) if DENSE_SPECS[name].get("dsp_block") == "mfe" else (-3.0, 3.0)
    r = np.random.default_rng(INPUT_SEED).uniform(lo, hi, (N_INPUTS - N_SYNTH, f.shape[1])).astype(np.float32)
    return np.ascontiguousarray(np.concatenate([f, r]), np.float32)


def graph_layout(blob):
    """(tensors, nodes, ids of the hidden FULLY_CONNECTED outputs in graph order, id of the last one's output, id of every MAX_POOL_2D-or-block output
    the pooled tap holds) -- the pooled tap of kws_nn_batch_device is those block outputs, then the hidden tensors"""
    tens, nodes, t_in, t_out, _ = eon_import.parse_blob(blob)
    fcs = [nd for nd in nodes if nd["op"] == 4]
    return tens, nodes, [nd["out"][0] for nd in fcs[:-1]], fcs[-1]["out"][0], t_in, t_out


def block_outputs(blob):
    """ids of the tensors that hold each conv block's (pooled) output, in graph order: what feeds the next CONV_2D / DEPTHWISE_CONV_2D or the first
    FULLY_CONNECTED (through RESHAPEs, which keep the bytes) -- the conv blocks' share of kws_nn_batch_device's tap_pooled"""
    _, nodes, _, _, _ = eon_import.parse_blob(blob)
    heads = [nd for nd in nodes if nd["op"] in (1, 6)]
    if not heads:
        return []
    first_fc = [nd for nd in nodes if nd["op"] == 4][0]
    return [nd["in"][0] for nd in heads[1:]] + [first_fc["in"][0]]


def clamp_bounds(tens, nodes, h):
    """(lo, hi) int8 values the fused activation of hidden tensor h's FULLY_CONNECTED clamps to (the non-vacuity conditions count entries on them)"""
    fc = [nd for nd in nodes if nd["op"] == 4 and nd["out"][0] == h][0]
    lo, hi = -128, 127
    sc, zp = tens[h]["scale"][0], tens[h]["zero"][0]
    if fc["p"][0] == 1:
        lo = max(lo, zp)
    elif fc["p"][0] == 2:
        lo, hi = max(lo, zp + int(round(-1.0 / sc))), min(hi, zp + int(round(1.0 / sc)))
    elif fc["p"][0] == 3:
        lo, hi = max(lo, zp), min(hi, zp + int(round(6.0 / sc)))
    return lo, hi


def check_not_vacuous(name, tens, nodes, hidden, taps, out_rows, f_rows):
    """the non-vacuity conditions of a DENSE_SPECS model, on int8 hidden tensors {id: [n][units]} and the two graphs' output rows; AssertionError otherwise"""
    for h in hidden:
        v = taps[h]
        lo, hi = clamp_bounds(tens, nodes, h)
        need = 8 if v.shape[1] == 1 else 16
        assert len(np.unique(v)) >= need, "%s: hidden tensor %d takes %d values" % (name, h, len(np.unique(v)))
        assert np.mean((v <= lo) | (v >= hi)) <= 0.5, "%s: more than half of hidden tensor %d sits on a clamp bound" % (name, h)
    assert len(np.unique(out_rows, axis=0)) >= 8 and len(np.unique(f_rows, axis=0)) >= 8, "%s: fewer than 8 distinct score rows" % name


def oracle_int8(oracle, blob, feats):
    """the oracle's network on each feature row: (q_in [n][F], {tensor id: [n][size] int8} for the hidden tensors and the logits, out_q [n][labels],
    scores [n][labels])"""
    m = oracle_model(oracle, blob)
    _, _, hidden, last, _, _ = graph_layout(blob)
    q = np.stack([m.quantize_input(f) for f in feats])
    taps = {i: [] for i in hidden + [last] + block_outputs(blob)}
    outs = []
    for row in q:
        out, tp = m.nn_invoke(row, taps=True)
        outs.append(out)
        for i in taps:
            taps[i].append(tp[i].copy())
    outs = np.stack(outs)
    return q, {i: np.stack(v) for i, v in taps.items()}, outs, np.stack([m.dequantize(o) for o in outs])


def oracle_f32(oracle, blob, feats):
    """float twin: ({tensor id: [n][size] float32} for the hidden tensors and the logits, scores [n][labels])"""
    m = oracle_model(oracle, blob)
    _, _, hidden, last, _, _ = graph_layout(blob)
    taps = {i: [] for i in hidden + [last]}
    outs = []
    for row in feats:
        out, tp = m.nn_invoke_f32(row, taps=True)
        outs.append(out)
        for i in taps:
            taps[i].append(tp[i].copy())
    return {i: np.stack(v) for i, v in taps.items()}, np.stack(outs)


def digest(a):
    """the first 8 bytes of the SHA-256 of an array's bytes (the fixture keeps one per hidden tensor)"""
    import hashlib
    return int.from_bytes(hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest()[:8], "little")
