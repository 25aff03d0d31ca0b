#!/usr/bin/env python3
"""Synthetic members of the Edge Impulse 1-D CNN graph family, as .kwsm blobs (tools/eon_import.py layout).

The reference ships two int8 models, both 32 mel filters / 13 cepstra.  BASELINE.json's other configurations
("40-band MFCC (49x40) + 2-Conv CNN, fp32", ...) have NO model file in the reference, so their
models are generated here: same graph (RESHAPE/CONV_2D/ADD/MAX_POOL_2D/FULLY_CONNECTED/SOFTMAX), seeded random int8
weights and quantisation parameters; tools/dequantize_model.py turns one into its float32 twin.  The parity tests use
the same generator for other widths / taps / pools / label counts.

    python tools/synth_model.py models/cfg2_mfcc40_int8.kwsm --seed 40 --num-filters 40 --ncep 40 --low 300 --high 0
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import eon_import  # noqa: E402

def dequantised_constants(tensors):
    """float64 value of every constant tensor of an int8 graph: (q - zero_point[ch]) * scale[ch] (what tools/dequantize_model.py stores)"""
    out = {}
    for i, t in enumerate(tensors):
        if not t["const"] or not t["scale"]:
            continue
        q = np.frombuffer(t["data"], np.int8 if t["type"] == 9 else np.int32).astype(np.float64).reshape(t["dims"])
        scale, zero = np.float64(t["scale"]), np.float64(t["zero"])
        if len(scale) > 1:
            shape = [1] * len(t["dims"])
            shape[t["qdim"]] = len(scale)
            out[i] = (q - zero.reshape(shape)) * scale.reshape(shape)
        else:
            out[i] = (q - zero[0]) * scale[0]
    return out


def is_residual(tensors, nodes):
    """an ADD of two activation tensors makes a graph residual"""
    return any(nd["op"] == 2 and not tensors[nd["in"][0]]["const"] and not tensors[nd["in"][1]]["const"] for nd in nodes)


def float_forward(tensors, nodes, t_in, x, stop_before_op=None, on_output=None, four_d=None):
    """The graph's float32 twin evaluated in numpy for a batch x [n][features] -- the arithmetic of the reference's float kernels
    (TFL/kernels/internal/reference/conv.h:28-99, depthwiseconv_float.h:25, add.h:179-215, pooling.h:189-237, fully_connected.h:26-60)
    without their rounding order: used to CALIBRATE a synthetic head, never as a checker.  Activations are kept as [n][time][channel];
    RESHAPE only renames axes in this graph family.  Returns {tensor id: value}; stops before the first node whose op is stop_before_op.
    A residual graph (is_residual; four_d says so for a slice of one) is a DAG: t_in may be a dict {tensor id: value} of the activations a slice of the
    graph starts from, every 4-D tensor is kept as [n][H][W][C] (H = 1 included), and ADD sums two activations."""
    act = {k: np.asarray(v, np.float64) for k, v in t_in.items()} if isinstance(t_in, dict) else {t_in: np.asarray(x, np.float64)}
    if four_d is None:
        four_d = is_residual(tensors, nodes)

    def fused(v, a):                                    # TfLiteFusedActivation: 0 none, 1 relu, 2 relu_n1_to_1, 3 relu6
        return v if a == 0 else np.maximum(v, 0.0) if a == 1 else np.clip(v, -1.0, 1.0) if a == 2 else np.clip(v, 0.0, 6.0)

    def windows(v, size, out_w, stride, pad_left, dil=1):      # [n][out_w][size][c], rows outside the image = NaN (callers mask them)
        n, w, c = v.shape
        idx = np.arange(out_w)[:, None] * stride - pad_left + np.arange(size)[None, :] * dil
        ok = (idx >= 0) & (idx < w)
        g = v[:, np.clip(idx, 0, w - 1), :]
        return g, ok

    def out_pad(size, k, stride, padding):             # kernels/padding.h: (output size, padding in front); a negative total is 0
        out = (size + stride - 1) // stride if padding == 1 else (size - k) // stride + 1
        return out, max(0, (out - 1) * stride + k - size) // 2

    def padded2d(v, kh, kw, sh, sw, padding, fill):    # [n][H][W][C] behind its padding, large enough for every window of every output
        n, hh, ww, c = v.shape
        (oh, pt), (ow, pl) = out_pad(hh, kh, sh, padding), out_pad(ww, kw, sw, padding)
        ap = np.full((n, max(pt + hh, (oh - 1) * sh + kh), max(pl + ww, (ow - 1) * sw + kw), c), fill, np.float64)
        ap[:, pt:pt + hh, pl:pl + ww] = v
        return ap, oh, ow

    for nd in nodes:
        if nd["op"] == stop_before_op:
            break
        const = dequantised_constants(tensors)          # per node: on_output may have re-quantised a bias
        o, p = nd["out"][0], nd["p"]
        dims = tensors[o]["dims"]
        a = act.get(nd["in"][0])
        if nd["op"] == 0:                               # RESHAPE
            n = a.shape[0]
            if len(dims) == 4 and ((dims[1] > 1 and dims[2] > 1) or four_d):          # a 2-D image [n][H][W][C] (blocks2d=, residual=)
                act[o] = a.reshape(n, dims[1], dims[2], dims[3])
            else:
                act[o] = a.reshape(n, -1) if len(dims) == 2 else a.reshape(n, -1, dims[-1])
        elif nd["op"] == 1 and a.ndim == 4:             # CONV_2D over both axes: filter [O][KH][KW][C], stride (p[2], p[1]), no dilation
            w = const[nd["in"][1]]
            b = const[nd["in"][2]] if len(nd["in"]) > 2 and nd["in"][2] >= 0 else 0.0
            kh, kw, sh, sw = w.shape[1], w.shape[2], p[2], p[1]
            ap, oh, ow = padded2d(a, kh, kw, sh, sw, p[0], 0.0)
            v = np.zeros((a.shape[0], oh, ow, w.shape[0]))
            for fy in range(kh):
                for fx in range(kw):
                    v += np.einsum("nhwc,oc->nhwo", ap[:, fy:fy + (oh - 1) * sh + 1:sh, fx:fx + (ow - 1) * sw + 1:sw], w[:, fy, fx])
            act[o] = fused(v + b, p[3])
        elif nd["op"] == 3 and a.ndim == 4:             # MAX_POOL_2D over both axes: window (p[4], p[3]), stride (p[2], p[1])
            ph, pw, sh, sw = p[4], p[3], p[2], p[1]
            ap, oh, ow = padded2d(a, ph, pw, sh, sw, p[0], -np.inf)
            v = np.full((a.shape[0], oh, ow, a.shape[3]), -np.inf)
            for fy in range(ph):
                for fx in range(pw):
                    v = np.maximum(v, ap[:, fy:fy + (oh - 1) * sh + 1:sh, fx:fx + (ow - 1) * sw + 1:sw])
            act[o] = fused(v, p[5])
        elif nd["op"] == 6 and a.ndim == 4:             # DEPTHWISE_CONV_2D over both axes: filter [1][KH][KW][C * p[6]], stride (p[2], p[1]), no dilation
            w = const[nd["in"][1]]
            b = const[nd["in"][2]] if len(nd["in"]) > 2 and nd["in"][2] >= 0 else 0.0
            kh, kw, sh, sw = w.shape[1], w.shape[2], p[2], p[1]
            ap, oh, ow = padded2d(a, kh, kw, sh, sw, p[0], 0.0)
            ap = np.repeat(ap, p[6], axis=3)             # output channel oc reads input channel oc // multiplier
            v = np.zeros((a.shape[0], oh, ow, w.shape[3]))
            for fy in range(kh):
                for fx in range(kw):
                    v += ap[:, fy:fy + (oh - 1) * sh + 1:sh, fx:fx + (ow - 1) * sw + 1:sw] * w[0, fy, fx]
            act[o] = fused(v + b, p[3])
        elif nd["op"] in (1, 6):                        # CONV_2D / DEPTHWISE_CONV_2D, 1 x K, stride p[1] and dilation p[4] along time
            w = const[nd["in"][1]]
            b = const[nd["in"][2]] if len(nd["in"]) > 2 and nd["in"][2] >= 0 else 0.0
            n, in_w, in_c = a.shape
            taps = w.shape[2]
            stride, dil = p[1], p[4]
            eff = (taps - 1) * dil + 1                   # kernels/padding.h: ComputeOutSize, ComputePaddingWithOffset (a negative total is 0)
            out_w = (in_w + stride - 1) // stride if p[0] == 1 else (in_w + stride - eff) // stride
            pad_left = max(0, (out_w - 1) * stride + eff - in_w) // 2
            g, ok = windows(a, taps, out_w, stride, pad_left, dil)
            g = np.where(ok[None, :, :, None], g, 0.0)
            if nd["op"] == 1:
                v = np.einsum("nwtc,otc->nwo", g, w[:, 0]) + b
            else:
                mult = p[6]
                v = np.einsum("nwto,to->nwo", np.repeat(g, mult, axis=3), w[0, 0]) + b
            act[o] = fused(v, p[3])
        elif nd["op"] == 2 and nd["in"][1] in act:      # ADD of two activations (a residual graph)
            act[o] = fused(a + act[nd["in"][1]], p[0])
        elif nd["op"] == 2:                             # ADD of a per-channel constant
            act[o] = fused(a + const[nd["in"][1]], p[0])
        elif nd["op"] == 3:                             # MAX_POOL_2D over time
            n, in_w, c = a.shape
            size, stride = p[4], p[2]
            out_w = dims[1]
            pad_left = max(0, (out_w - 1) * stride + size - in_w) // 2 if p[0] == 1 else 0
            g, ok = windows(a, size, out_w, stride, pad_left)
            act[o] = fused(np.where(ok[None, :, :, None], g, -np.inf).max(axis=2), p[5])
        elif nd["op"] == 4:                             # FULLY_CONNECTED
            bias = const[nd["in"][2]] if len(nd["in"]) > 2 and nd["in"][2] >= 0 else 0.0          # FULLY_CONNECTED's bias is optional
            act[o] = fused(a @ const[nd["in"][1]].T + bias, p[0])
        elif nd["op"] == 5:                             # SOFTMAX
            e = np.exp((a - a.max(axis=1, keepdims=True)) * nd["beta"])
            act[o] = e / e.sum(axis=1, keepdims=True)
        else:
            raise ValueError("op %d" % nd["op"])
        if on_output:
            on_output(nd, act[o])
    return act


def calibrate_ranges(tensors, nodes, t_in, x):
    """Post-training quantisation of a synthetic graph's ACTIVATIONS: the drawn activation scales / zero points are arbitrary, so the int8
    graph clamps most of what flows through it and has little to do with its float twin.  Here every CONV_2D / DEPTHWISE_CONV_2D / ADD /
    FULLY_CONNECTED output gets the range its float twin shows on the calibration set x (min .. max, including 0), RESHAPE and
    MAX_POOL_2D outputs keep their input's parameters (as TFLite requires), and every int32 bias is re-quantised at its new scale
    input scale x filter scale[ch] (kernel_util_lite.cc:47-120 checks that product) from its old float value.  Weights and the input
    tensor keep their drawn parameters."""
    def on_output(nd, v):
        o, i0 = nd["out"][0], nd["in"][0]
        if nd["op"] in (0, 3):
            tensors[o]["scale"], tensors[o]["zero"] = list(tensors[i0]["scale"]), list(tensors[i0]["zero"])
            return
        if nd["op"] == 5:
            return
        lo, hi = min(float(v.min()), 0.0), max(float(v.max()), 0.0)
        sc = float(np.float32((hi - lo) / 255.0))
        tensors[o]["scale"], tensors[o]["zero"] = [sc], [int(np.clip(round(-128 - lo / sc), -128, 127))]

    def before(nd):                                     # the bias of a node whose input scale has just been settled
        if nd["op"] not in (1, 4, 6) or len(nd["in"]) < 3 or nd["in"][2] < 0:
            return
        tb, tw, i0 = nd["in"][2], nd["in"][1], nd["in"][0]
        old = np.frombuffer(tensors[tb]["data"], np.int32).astype(np.float64) * np.float64(tensors[tb]["scale"])
        new_scale = [float(np.float32(tensors[i0]["scale"][0]) * np.float32(s_)) for s_ in tensors[tw]["scale"]]
        tensors[tb]["scale"] = new_scale
        tensors[tb]["data"] = np.round(old / np.float64(new_scale)).astype(np.int32).tobytes()

    # a node's inputs come from the activations so far, not from "the previous output": the graph may be a DAG (residual=)
    act = {t_in: np.asarray(x, np.float64)}
    four_d = is_residual(tensors, nodes)
    for nd in nodes:
        before(nd)
        if nd["op"] == 5:
            break
        sub = float_forward(tensors, [nd], {k: act[k] for k in nd["in"] if k in act}, None, on_output=on_output, four_d=four_d)
        act[nd["out"][0]] = sub[nd["out"][0]]


def calibrate_residual(tensors, nodes, t_in, x, lift=0.5, lifts=None, per_tensor=False):
    """The convolutions of a residual graph (synth_model_blob's residual=), in node order on the calibration set x.  As drawn, a ReLU parks about half of a
    convolution's outputs on its bound and the drawn output scales saturate the rest, so that every ADD sums two clamped tensors.  Per convolution: a
    ReLU_N1_TO_1 / ReLU6 one gets weight scales that make its pre-activations' deviation 0.5 / 1.5; the int32 bias is set per channel so that the float
    twin's pre-activation has mean lift x its own deviation under ReLU / ReLU6 (about 0.5: a third of the outputs below zero) and mean 0 otherwise
    (lifts: {node index: lift} overrides that for a node, whatever its activation).  Then every activation range is settled (calibrate_ranges)."""
    four_d = True
    for idx, nd in enumerate(nodes):
        if nd["op"] not in (1, 6):
            continue
        calibrate_ranges(tensors, nodes[:idx], t_in, x)
        a = float_forward(tensors, nodes[:idx], t_in, x, four_d=four_d)[nd["in"][0]]
        tw = tensors[nd["in"][1]]
        has_bias = len(nd["in"]) > 2 and nd["in"][2] >= 0
        tb = tensors[nd["in"][2]] if has_bias else {"data": b""}               # (a depthwise step without a bias tensor: only its weight scales are set)
        if per_tensor:
            tw["scale"], tw["zero"] = [float(np.float32(np.mean(tw["scale"])))], [0]
        act = nd["p"][3]
        nd["p"][3] = 0                                   # the pre-activation: this node without its clamp and bias
        tb["data"] = bytes(len(tb["data"]))

        def pre():
            v = float_forward(tensors, [nd], {nd["in"][0]: a}, None, four_d=four_d)[nd["out"][0]]
            return v.reshape(-1, v.shape[-1])
        if act in (2, 3):
            sd = pre().std()
            tw["scale"] = [float(np.float32(s_ * (1.5 if act == 3 else 0.5) / sd)) for s_ in tw["scale"]]
        v = pre()
        nd["p"][3] = act
        if not has_bias:
            continue
        in_scale = tensors[nd["in"][0]]["scale"][0]
        tb["scale"] = [float(np.float32(in_scale) * np.float32(s_)) for s_ in tw["scale"]]
        tb["zero"] = [0] * len(tb["scale"])
        k = (lifts or {}).get(idx, lift if act in (1, 3) else 0.0)
        bias = np.round((k * v.std(axis=0) - v.mean(axis=0)) / np.float64(tb["scale"]))
        assert np.abs(bias).max() < 2 ** 31
        tb["data"] = bias.astype(np.int32).tobytes()
    fc = [i for i, nd in enumerate(nodes) if nd["op"] == 4][0]
    calibrate_ranges(tensors, nodes[:fc], t_in, x)


def calibrate_hidden(tensors, nodes, t_in, hidden, x, lift=0.7):
    """Hidden FULLY_CONNECTED layers of a synthetic dense stack (synth_model_blob's dense=): as drawn, a layer's pre-activations have zero mean over
    the inputs, so a ReLU parks half of its outputs on the clamp bound, and the drawn output scale saturates the rest -- every clip then produces the
    same tensor and a test on such a graph proves nothing.  Layer by layer, on the calibration set x: the activation ranges in front of the layer are
    settled (calibrate_ranges), then every unit's int32 bias is set so that its float twin's pre-activation has mean lift x its own deviation (about a
    quarter of the outputs below zero).  The layer's own output range is settled by the calibrate_ranges pass that follows (calibrate_head)."""
    for fc in hidden:
        idx = nodes.index(fc)
        calibrate_ranges(tensors, nodes[:idx], t_in, x)
        a = float_forward(tensors, nodes[:idx], t_in, x)[fc["in"][0]]
        tw, tb = fc["in"][1], fc["in"][2]
        z = a.reshape(a.shape[0], -1) @ dequantised_constants(tensors)[tw].T
        b_scale = float(np.float32(tensors[fc["in"][0]]["scale"][0]) * np.float32(tensors[tw]["scale"][0]))
        bias = np.round((lift * z.std(axis=0) - z.mean(axis=0)) / b_scale).astype(np.int64)
        assert np.abs(bias).max() < 2 ** 31
        tensors[tb]["scale"] = [b_scale]
        tensors[tb]["data"] = bias.astype(np.int32).tobytes()


def calibrate_head(tensors, nodes, t_in, tfw, tfb, tfo, logit_std, seed, n_cal=256, x=None):
    """Give a synthetic graph a head with a sane logit scale (synth_model_blob's logit_std).  The network's input is cmvnw's output:
    every column standardised over its window -- so the calibration set is n_cal matrices of independent N(0, 1) values (measured: the
    logit statistics on those equal the ones on the bench's synthetic clips to a few percent).  With z = W x the float twin's
    bias-free logits on that set: the FULLY_CONNECTED weight scale is multiplied by logit_std / pooled deviation of (z - class mean), the
    int32 biases become round(-class mean / bias scale) + the drawn ones, and the output tensor's scale spans +-8 logit_std."""
    rng = np.random.default_rng(100000 + seed)
    F = tensors[t_in]["dims"][1]
    if x is None:
        x = rng.standard_normal((n_cal, F))
    fc = [nd for nd in nodes if nd["op"] == 4][-1]          # the head: the last FULLY_CONNECTED (the only one without dense=)
    calibrate_ranges(tensors, nodes, t_in, x)
    feat = float_forward(tensors, nodes[:nodes.index(fc)], t_in, x)[fc["in"][0]]
    w = dequantised_constants(tensors)[tfw]
    z = feat @ w.T
    mean = z.mean(axis=0)
    k = logit_std / float(np.sqrt(((z - mean) ** 2).mean()))
    fw_scale = float(np.float32(tensors[tfw]["scale"][0] * k))
    b_scale = float(np.float32(tensors[fc["in"][0]]["scale"][0]) * np.float32(fw_scale))
    drawn = np.frombuffer(tensors[tfb]["data"], np.int32)
    bias = np.round(-mean * k / b_scale).astype(np.int64) + drawn
    assert np.abs(bias).max() < 2 ** 31
    tensors[tfw]["scale"] = [fw_scale]
    tensors[tfb]["scale"] = [b_scale]
    tensors[tfb]["data"] = bias.astype(np.int32).tobytes()
    tensors[tfo]["scale"] = [float(np.float32(logit_std * 8.0 / 128.0))]


def synth_model_blob(seed, ncep=13, win_size=101, low=300, high=4000, blocks=((30, 7, 7), (10, 7, 7)), n_labels=4,
                     conv_bias=False, add_bias=True, num_filters=32, raw_samples=16000, fft_length=256, frame_length=0.02,
                     frame_stride=0.02, pre_cof=0.98, dsp_block="mfcc", logit_std=None, quantize_filterbank=False, edit=None, dense=None,
                     calib=None, conv_valid=(), conv_stride=None, conv_dilation=None, blocks2d=None, residual=None, two_d=False, residual_opts=None):
    """blocks: sequence of
         (out_channels, taps, pool)              CONV_2D 1xK (+ optional int32 bias) -> ADD(int8 per-channel)+ReLU -> MAX_POOL
         ("dw", depth_mult, taps, pool, act)     DEPTHWISE_CONV_2D 1xK with int32 bias and fused activation -> MAX_POOL
         ("pw", out_channels, act)               CONV_2D 1x1 with int32 bias and fused activation (pointwise)
       (pool 1 = no pooling node, a negative pool = VALID padding: the ragged tail of the time axis is dropped; act: TfLiteFusedActivation 0 none, 1 relu, 3 relu6).
       A pool may also be a tuple (window, stride, valid): a MAX_POOL_2D whose stride differs from its window (overlapping or skipping windows), with
       VALID (valid true) or SAME padding.  conv_valid: indices into blocks of the convolutions with VALID padding (output rows = rows - taps + 1)
       instead of SAME.  conv_stride / conv_dilation: {index into blocks: stride_w / dilation_width_factor} of the convolutions (all three block kinds)
       that stride or dilate along time; the output rows follow kernels/padding.h (SAME: ceil(rows / stride); VALID: (rows - ((taps - 1) * dilation + 1))
       // stride + 1).  None of these draws anything: with integer pools, conv_valid=() and neither dict given every blob is the one the same arguments
       gave before.
       logit_std: None = the FULLY_CONNECTED layer as drawn (random weights and biases: one class usually wins every clip by tens
       of logit units, the softmax is saturated and a score says nothing about the logits behind it); a number = the head is
       calibrated (calibrate_head): scale and biases are set so that, over standardised random feature matrices -- which is what
       cmvnw hands the network --, every class's logit has zero mean and the logits' pooled deviation is logit_std (the shipped
       impulse's is 1.5).  No random draw is added or removed: every other tensor is the one the same seed gave before.
       Frame geometry defaults to the shipped one (1 s at 16 kHz, 20 ms frames and stride: 49 frames); raw_samples / frame_length /
       frame_stride / fft_length / pre_cof change the DSP block (the frame count follows speechpy's rule, processing.hpp:260-284).
       blocks=() is a dense-only classifier on the feature matrix.  dense: None, or a sequence of (units, act) -- hidden FULLY_CONNECTED layers (int32
       bias, fused activation act) between the flattened output of the last block and the head.  A graph with hidden layers is always calibrated
       (calibrate_hidden, then calibrate_head with logit_std or 1.5) on standardised random feature matrices, or on calib ([n][features]) where the
       DSP block's output is not of that kind (the MFE block's).  With dense=None every blob is the one the same arguments gave before.
       blocks2d: None, or the blocks of a 2-D convolutional graph (Edge Impulse's "2D Convolutional" classifier), which then REPLACE blocks: the features are
       reshaped to [1][frames][columns][1] and every block is (out_channels, kh, kw, pool) or (out_channels, kh, kw, pool, options) -- a CONV_2D kh x kw with
       int32 bias and fused ReLU, then MAX_POOL_2D pool x pool at stride pool, SAME padding (pool 0 / 1: no pooling node).  options (a dict): stride=(h, w),
       valid=True (VALID convolution), act=0 .. 3, bias=False (no bias tensor), pool=(h, w) window, pool_stride=(h, w), pool_valid=True.  A flatten, dense=,
       the head and softmax follow as ever.  It draws nothing when blocks2d is None: every blob is the one the same arguments gave before.
       residual: None, or the steps of a residual graph, which then REPLACE blocks: the features are reshaped to [1][1][frames][columns] (two_d:
       [1][frames][columns][1]) -- the tensor named "in" -- and every step names its output:
         (name, "conv", src, out_c, kh, kw, (sh, sw), valid, act[, lift])   CONV_2D kh x kw on tensor src with int32 bias and fused activation act
         (name, "dw", src, depth_multiplier, kh, kw, (sh, sw), valid, act[, lift])   DEPTHWISE_CONV_2D kh x kw on tensor src: filter
                                                                            [1][kh][kw][channels x depth_multiplier], per-channel scales along dimension 3
         (name, "add", a, b, act)                                           ADD of tensors a and b (the same name twice is allowed)
         (name, "pool", src, (ph, pw), (psh, psw), valid[, keras])           MAX_POOL_2D; keras: through the [1][W][1][C] renaming of Keras' Conv1D exports
       The last step's output is flattened; dense=, the head and softmax follow as ever.  Such a graph is always calibrated (calibrate_residual on
       standardised random feature matrices or calib: the bias of an activated convolution lifts its pre-activations by 0.5 deviations -- a step's own lift
       overrides that --, every step output gets the range its float twin shows; then calibrate_hidden / calibrate_head).  residual_opts: dict(per_tensor=True)
       gives every filter ONE scale; dict(no_bias=(names)) leaves the named depthwise steps without a bias tensor.  With two_d=True and a "dw" step no ADD is
       needed: the step trunks serve such a graph too.  A "dw" step draws only its own constants: every spec without one gives the blob it gave before.
       It draws nothing when residual is None: every blob is the one the same arguments gave before.
       edit: a callable edit(tensors, nodes) run on the finished graph just before it is serialised -- the way to any quantisation
       parameter, constant or node option outside the drawn bands (tests/kws_testlib.py QUANT_EDGES).  It draws nothing from the
       model's generator: with edit=None every blob is the one the same arguments gave before."""
    rng = np.random.default_rng(seed)
    flen_s = int(round(16000 * np.float32(frame_length)))
    n_frames = int(np.floor(np.float32(raw_samples - flen_s) / np.float32(round(16000 * np.float32(frame_stride)))))
    assert n_frames >= 1
    if dsp_block == "mfe":          # extract_mfe_features: the feature matrix is [frames][mel filters]
        ncep = num_filters
    F = n_frames * ncep
    tensors, nodes = [], []

    def T(ttype, dims, const=False, scale=(), zero=(), data=b"", qdim=0):
        nbytes = int(np.prod(dims)) * {1: 4, 2: 4, 9: 1}[ttype]
        if const:
            assert len(data) == nbytes
        tensors.append({"type": ttype, "dims": list(dims), "nbytes": nbytes, "const": const, "scale": list(scale),
                        "zero": list(zero), "qdim": qdim, "data": data})
        return len(tensors) - 1

    def node(op, ins, outs, p=None, beta=0.0):
        pp = [0] * 8
        if p:
            pp[:len(p)] = p
        nodes.append({"op": op, "in": list(ins), "out": list(outs), "p": pp, "beta": beta})

    def shape_const(dims):
        return T(2, [len(dims)], True, data=np.int32(dims).tobytes())

    def rscale(lo, hi):
        return float(np.float32(np.exp(rng.uniform(np.log(lo), np.log(hi)))))

    residual_lift = {}                                  # residual=: node index -> a convolution's own lift
    in_scale, in_zp = rscale(0.03, 0.06), int(rng.integers(-20, 5))
    t_in = T(9, [1, F], scale=[in_scale], zero=[in_zp])
    cur, cur_scale, cur_zp, w, c = t_in, in_scale, in_zp, n_frames, ncep
    if residual is not None:
        blocks = ()
        hh, ww, cc = (n_frames, ncep, 1) if two_d else (1, n_frames, ncep)
        t = T(9, [1, hh, ww, cc], scale=[cur_scale], zero=[cur_zp])
        node(0, [cur, shape_const([1, hh, ww, cc])], [t])
        named = {"in": (t, hh, ww, cc)}                                 # name -> (tensor id, H, W, C)
        no_bias = tuple((residual_opts or {}).get("no_bias", ()))       # names of the depthwise steps without a bias tensor (a two-input node)

        def drawn_output(act):
            return rscale(0.03, 0.12), int(rng.integers(-128, -90)) if act in (1, 3) else int(rng.integers(-30, 40))

        for ent in residual:
            name, kind = ent[0], ent[1]
            assert name not in named, name
            if kind == "conv":
                src, oc, kh, kw, (sh, sw), valid, act = ent[2:9]
                ts, h_, w_, c_ = named[src]
                wq = rng.integers(-127, 128, (oc, kh, kw, c_)).astype(np.int8)
                wscales = [rscale(0.001, 0.005) for _ in range(oc)]
                tw = T(9, [oc, kh, kw, c_], True, wscales, [0] * oc, wq.tobytes())
                bias = rng.integers(-300, 300, oc).astype(np.int32)
                tb = T(2, [oc], True, [tensors[ts]["scale"][0] * s_ for s_ in wscales], [0] * oc, bias.tobytes())
                out_scale, out_zp = drawn_output(act)
                if valid:                                               # ComputeOutSize (kernels/padding.h)
                    assert h_ >= kh and w_ >= kw
                    h_, w_ = (h_ - kh) // sh + 1, (w_ - kw) // sw + 1
                else:
                    h_, w_ = (h_ + sh - 1) // sh, (w_ + sw - 1) // sw
                tc = T(9, [1, h_, w_, oc], scale=[out_scale], zero=[out_zp])
                node(1, [ts, tw, tb], [tc], [2 if valid else 1, sw, sh, act, 1, 1])
                if len(ent) > 9:
                    residual_lift[len(nodes) - 1] = ent[9]
                named[name] = (tc, h_, w_, oc)
            elif kind == "dw":
                src, mult, kh, kw, (sh, sw), valid, act = ent[2:9]
                ts, h_, w_, c_ = named[src]
                oc = c_ * mult
                wq = rng.integers(-127, 128, (1, kh, kw, oc)).astype(np.int8)
                wscales = [rscale(0.002, 0.02) for _ in range(oc)]
                tw = T(9, [1, kh, kw, oc], True, wscales, [0] * oc, wq.tobytes(), qdim=3)
                bias = rng.integers(-300, 300, oc).astype(np.int32)
                ins = [ts, tw]
                if name not in no_bias:
                    ins.append(T(2, [oc], True, [tensors[ts]["scale"][0] * s_ for s_ in wscales], [0] * oc, bias.tobytes()))
                out_scale, out_zp = drawn_output(act)
                if valid:                                               # ComputeOutSize (kernels/padding.h)
                    assert h_ >= kh and w_ >= kw
                    h_, w_ = (h_ - kh) // sh + 1, (w_ - kw) // sw + 1
                else:
                    h_, w_ = (h_ + sh - 1) // sh, (w_ + sw - 1) // sw
                tc = T(9, [1, h_, w_, oc], scale=[out_scale], zero=[out_zp])
                node(6, ins, [tc], [2 if valid else 1, sw, sh, act, 1, 1, mult])
                if len(ent) > 9:
                    residual_lift[len(nodes) - 1] = ent[9]
                named[name] = (tc, h_, w_, oc)
            elif kind == "add":
                a_, b_, act = ent[2:5]
                (ta, h_, w_, c_), (tb_, hb, wb, cb) = named[a_], named[b_]
                assert (h_, w_, c_) == (hb, wb, cb), (name, named[a_], named[b_])
                out_scale, out_zp = drawn_output(act)
                to = T(9, [1, h_, w_, c_], scale=[out_scale], zero=[out_zp])
                node(2, [ta, tb_], [to], [act])
                named[name] = (to, h_, w_, c_)
            elif kind == "pool":
                src, (ph, pw), (psh, psw), valid = ent[2:6]
                keras = len(ent) > 6 and ent[6]                         # through the [1][W][1][C] renaming of Keras' Conv1D exports (1-D graphs)
                ts, h_, w_, c_ = named[src]
                q = dict(scale=list(tensors[ts]["scale"]), zero=list(tensors[ts]["zero"]))
                if valid:
                    assert h_ >= ph and w_ >= pw
                    h2, w2, pad = (h_ - ph) // psh + 1, (w_ - pw) // psw + 1, 2
                else:
                    h2, w2, pad = (h_ + psh - 1) // psh, (w_ + psw - 1) // psw, 1
                if keras:
                    assert h_ == 1 and ph == 1 and psh == 1
                    t4 = T(9, [1, w_, 1, c_], **q)
                    node(0, [ts, shape_const([1, w_, 1, c_])], [t4])
                    tp = T(9, [1, w2, 1, c_], **q)
                    node(3, [t4], [tp], [pad, 1, psw, 1, pw, 0])
                    t5 = T(9, [1, 1, w2, c_], **q)
                    node(0, [tp, shape_const([1, 1, w2, c_])], [t5])
                    tp = t5
                else:
                    tp = T(9, [1, h2, w2, c_], **q)
                    node(3, [ts], [tp], [pad, psw, psh, pw, ph, 0])
                named[name] = (tp, h2, w2, c_)
            else:
                raise ValueError("residual step kind %r" % (kind,))
        cur, hh, ww, c = named[residual[-1][0]]
        cur_scale, cur_zp = tensors[cur]["scale"][0], tensors[cur]["zero"][0]
        w = hh * ww                                                     # the flatten below: NHWC order
    elif blocks2d is not None:
        blocks = ()
        hh, w, c = n_frames, ncep, 1
        t = T(9, [1, hh, w, 1], scale=[cur_scale], zero=[cur_zp])
        node(0, [cur, shape_const([1, hh, w, 1])], [t])
        cur = t
        for blk in blocks2d:
            oc, kh, kw, pool = blk[:4]
            opt = dict(blk[4]) if len(blk) > 4 else {}
            (sh, sw), valid, act = opt.get("stride", (1, 1)), bool(opt.get("valid", False)), opt.get("act", 1)
            wq = rng.integers(-127, 128, (oc, kh, kw, c)).astype(np.int8)
            wscales = [rscale(0.001, 0.005) for _ in range(oc)]
            tw = T(9, [oc, kh, kw, c], True, wscales, [0] * oc, wq.tobytes())
            ins = [cur, tw]
            if opt.get("bias", True):
                bias = rng.integers(-300, 300, oc).astype(np.int32)
                ins.append(T(2, [oc], True, [cur_scale * s_ for s_ in wscales], [0] * oc, bias.tobytes()))
            out_scale, out_zp = rscale(0.03, 0.12), int(rng.integers(-128, -90)) if act in (1, 3) else int(rng.integers(-30, 40))
            if valid:                                                   # ComputeOutSize (kernels/padding.h)
                assert hh >= kh and w >= kw
                hh, w = (hh - kh) // sh + 1, (w - kw) // sw + 1
            else:
                hh, w = (hh + sh - 1) // sh, (w + sw - 1) // sw
            tc = T(9, [1, hh, w, oc], scale=[out_scale], zero=[out_zp])
            node(1, ins, [tc], [2 if valid else 1, sw, sh, act, 1, 1])
            cur, cur_scale, cur_zp, c = tc, out_scale, out_zp, oc
            ph, pw = opt.get("pool", (pool, pool) if pool > 1 else (1, 1))
            psh, psw = opt.get("pool_stride", (ph, pw))
            if (ph, pw) != (1, 1) or (psh, psw) != (1, 1):
                if opt.get("pool_valid", False):
                    assert hh >= ph and w >= pw
                    hh, w, pad = (hh - ph) // psh + 1, (w - pw) // psw + 1, 2
                else:
                    hh, w, pad = (hh + psh - 1) // psh, (w + psw - 1) // psw, 1
                tp = T(9, [1, hh, w, oc], scale=[cur_scale], zero=[cur_zp])
                node(3, [cur], [tp], [pad, psw, psh, pw, ph, 0])
                cur = tp
        w = hh * w                                                      # the flatten below: NHWC order
    else:
        t = T(9, [1, 1, w, c], scale=[cur_scale], zero=[cur_zp])
        node(0, [cur, shape_const([1, 1, w, c])], [t])
        cur = t
    def add_pool(pool):
        nonlocal cur, w
        if pool in (0, 1):
            return
        if isinstance(pool, tuple):                                     # (window, stride, valid)
            pool, stride, valid = pool
        else:
            valid = pool < 0                                            # negative: VALID padding (floor, a ragged tail is dropped)
            pool = stride = abs(pool)
        t4 = T(9, [1, w, 1, c_out], scale=[cur_scale], zero=[cur_zp])
        node(0, [cur, shape_const([1, w, 1, c_out])], [t4])
        pw = (w - pool) // stride + 1 if valid else (w + stride - 1) // stride      # ComputeOutSize (kernels/padding.h)
        assert pw >= 1 and (pw - 1) * stride < w         # SAME: the last window may be ragged (clipped to the tensor)
        tp = T(9, [1, pw, 1, c_out], scale=[cur_scale], zero=[cur_zp])
        node(3, [t4], [tp], [2 if valid else 1, 1, stride, 1, pool, 0])   # VALID / SAME, stride (w1,hP), filter (w1,hP)
        w = pw
        t5 = T(9, [1, 1, w, c_out], scale=[cur_scale], zero=[cur_zp])
        node(0, [tp, shape_const([1, 1, w, c_out])], [t5])
        cur = t5

    strides, dilations = dict(conv_stride or {}), dict(conv_dilation or {})
    assert all(0 <= bi < len(blocks) for bi in list(strides) + list(dilations))

    def conv_rows(bi, taps):                                                # TfLitePadding of block bi's convolution; w becomes its output rows
        nonlocal w
        s_, eff = strides.get(bi, 1), (taps - 1) * dilations.get(bi, 1) + 1
        assert 1 <= s_ <= w
        if bi in conv_valid:
            assert (w - eff) // s_ + 1 >= 1 and w >= eff
            w = (w - eff) // s_ + 1
            return 2
        w = (w + s_ - 1) // s_
        return 1

    for bi, blk in enumerate(blocks):
        if blk[0] == "dw":
            _, mult, taps, pool, act = blk
            c_out = c * mult
            wq = rng.integers(-127, 128, (1, 1, taps, c_out)).astype(np.int8)
            wscales = [rscale(0.002, 0.02) for _ in range(c_out)]
            tw = T(9, [1, 1, taps, c_out], True, wscales, [0] * c_out, wq.tobytes(), qdim=3)
            bias = rng.integers(-300, 300, c_out).astype(np.int32)
            tb = T(2, [c_out], True, [cur_scale * s_ for s_ in wscales], [0] * c_out, bias.tobytes())
            out_scale, out_zp = rscale(0.03, 0.12), int(rng.integers(-128, -90)) if act else int(rng.integers(-30, 40))
            padding = conv_rows(bi, taps)
            tc = T(9, [1, 1, w, c_out], scale=[out_scale], zero=[out_zp])
            node(6, [cur, tw, tb], [tc], [padding, strides.get(bi, 1), 1, act, dilations.get(bi, 1), 1, mult])    # SAME (or VALID)
            cur, cur_scale, cur_zp = tc, out_scale, out_zp
            add_pool(pool)
            c = c_out
            continue
        if blk[0] == "pw":
            _, c_out, act = blk
            wq = rng.integers(-127, 128, (c_out, 1, 1, c)).astype(np.int8)
            wscales = [rscale(0.001, 0.008) for _ in range(c_out)]
            tw = T(9, [c_out, 1, 1, c], True, wscales, [0] * c_out, wq.tobytes())
            bias = rng.integers(-300, 300, c_out).astype(np.int32)
            tb = T(2, [c_out], True, [cur_scale * s_ for s_ in wscales], [0] * c_out, bias.tobytes())
            out_scale, out_zp = rscale(0.03, 0.12), int(rng.integers(-128, -90)) if act else int(rng.integers(-30, 40))
            padding = conv_rows(bi, 1)
            tc = T(9, [1, 1, w, c_out], scale=[out_scale], zero=[out_zp])
            node(1, [cur, tw, tb], [tc], [padding, strides.get(bi, 1), 1, act, dilations.get(bi, 1), 1])
            cur, cur_scale, cur_zp = tc, out_scale, out_zp
            c = c_out
            continue
        (oc, taps, pool) = blk
        c_out = oc
        wq = rng.integers(-127, 128, (oc, 1, taps, c)).astype(np.int8)
        wscales = [rscale(0.001, 0.005) for _ in range(oc)]
        tw = T(9, [oc, 1, taps, c], True, wscales, [0] * oc, wq.tobytes())
        bias = rng.integers(-200, 200, oc).astype(np.int32) if conv_bias else np.zeros(oc, np.int32)
        tb = T(2, [oc], True, [cur_scale * s for s in wscales], [0] * oc, bias.tobytes())
        out_scale, out_zp = rscale(0.03, 0.12), int(rng.integers(-30, 40))
        padding = conv_rows(bi, taps)
        tc = T(9, [1, 1, w, oc], scale=[out_scale], zero=[out_zp])
        node(1, [cur, tw, tb], [tc], [padding, strides.get(bi, 1), 1, 0, dilations.get(bi, 1), 1])      # SAME (or VALID), no activation
        cur, cur_scale, cur_zp = tc, out_scale, out_zp
        if add_bias:
            t3 = T(9, [1, w, oc], scale=[cur_scale], zero=[cur_zp])
            node(0, [cur, shape_const([1, w, oc])], [t3])
            bq = rng.integers(-127, 1, oc).astype(np.int8)
            tbq = T(9, [oc], True, [rscale(0.001, 0.01)], [0], bq.tobytes())
            a_scale = rscale(0.02, 0.05)
            ta = T(9, [1, w, oc], scale=[a_scale], zero=[-128])
            node(2, [t3, tbq], [ta], [1])                                   # ReLU
            cur, cur_scale, cur_zp = ta, a_scale, -128
        if pool not in (0, 1):
            add_pool(pool)
        elif add_bias:                                                      # back to NHWC for the next convolution
            t6 = T(9, [1, 1, w, oc], scale=[cur_scale], zero=[cur_zp])
            node(0, [cur, shape_const([1, 1, w, oc])], [t6])
            cur = t6
        c = oc
    fc_in = w * c
    tf = T(9, [1, fc_in], scale=[cur_scale], zero=[cur_zp])
    node(0, [cur, shape_const([1, fc_in])], [tf])
    hidden = []
    for units, act in (dense or ()):
        hw = rng.integers(-127, 128, (units, fc_in)).astype(np.int8)
        hw_scale = rscale(0.002, 0.01)
        thw = T(9, [units, fc_in], True, [hw_scale], [0], hw.tobytes())
        thb = T(2, [units], True, [cur_scale * hw_scale], [0], rng.integers(-400, 400, units).astype(np.int32).tobytes())
        cur_scale, cur_zp = rscale(0.03, 0.12), (-128 if act in (1, 3) else int(rng.integers(-30, 40)))
        tho = T(9, [1, units], scale=[cur_scale], zero=[cur_zp])
        node(4, [tf, thw, thb], [tho], [act])
        hidden.append(nodes[-1])
        tf, fc_in = tho, units
    fw = rng.integers(-127, 128, (n_labels, fc_in)).astype(np.int8)
    fw_scale = rscale(0.005, 0.02)
    tfw = T(9, [n_labels, fc_in], True, [fw_scale], [0], fw.tobytes())
    tfb = T(2, [n_labels], True, [cur_scale * fw_scale], [0], rng.integers(-400, 400, n_labels).astype(np.int32).tobytes())
    tfo = T(9, [1, n_labels], scale=[rscale(0.05, 0.2)], zero=[int(rng.integers(-10, 10))])
    node(4, [tf, tfw, tfb], [tfo], [0])
    tso = T(9, [1, n_labels], scale=[0.00390625], zero=[-128])
    node(5, [tfo], [tso], beta=1.0)
    if residual is not None:
        xc = np.random.default_rng(200000 + seed).standard_normal((256, F)) if calib is None else np.asarray(calib, np.float64)
        calibrate_residual(tensors, nodes, t_in, xc, lifts=residual_lift, per_tensor=bool((residual_opts or {}).get("per_tensor")))
        calibrate_hidden(tensors, nodes, t_in, hidden, xc)
        calibrate_head(tensors, nodes, t_in, tfw, tfb, tfo, 1.5 if logit_std is None else float(logit_std), seed, x=xc)
    elif hidden:
        xc = np.random.default_rng(200000 + seed).standard_normal((256, F)) if calib is None else np.asarray(calib, np.float64)
        calibrate_hidden(tensors, nodes, t_in, hidden, xc)
        calibrate_head(tensors, nodes, t_in, tfw, tfb, tfo, 1.5 if logit_std is None else float(logit_std), seed, x=xc)
    elif logit_std is not None:
        calibrate_head(tensors, nodes, t_in, tfw, tfb, tfo, float(logit_std), seed, x=calib)
    if edit is not None:
        edit(tensors, nodes)
    meta = {"labels": ["label%d" % i for i in range(n_labels)],
            "dsp": {"axes": 1, "num_cepstral": ncep, "frame_length": frame_length, "frame_stride": frame_stride, "num_filters": num_filters,
                    "fft_length": fft_length, "win_size": win_size, "low_frequency": low, "high_frequency": high,
                    "pre_cof": pre_cof, "pre_shift": 1, "block": 1 if dsp_block == "mfe" else 0,
                    "quantize_filterbank": 1 if quantize_filterbank else 0},
            "raw_sample_count": raw_samples, "frequency": 16000, "nn_input_frame_size": F}
    return eon_import.serialise(tensors, nodes, t_in, tso, meta)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out")
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--ncep", type=int, default=13)
    ap.add_argument("--num-filters", type=int, default=32)
    ap.add_argument("--win-size", type=int, default=101)
    ap.add_argument("--low", type=int, default=300)
    ap.add_argument("--high", type=int, default=4000)
    ap.add_argument("--labels", type=int, default=4)
    ap.add_argument("--blocks", default="30,7,7;10,7,7", help="per block: out_channels,taps,pool | dw,depth_mult,taps,pool,act | pw,out_channels,act")
    ap.add_argument("--dense", default="", help="hidden FULLY_CONNECTED layers in front of the head: units,act;units,act (act: 0 none, 1 relu, 2 relu_n1_to_1, 3 relu6)")
    ap.add_argument("--logit-std", type=float, default=None, help="calibrate the head: zero-mean class logits of this pooled deviation on standardised features")
    ap.add_argument("--conv-stride", default="", help="strided convolutions: block:stride;block:stride (block: index into --blocks)")
    ap.add_argument("--conv-dilation", default="", help="dilated convolutions: block:dilation;block:dilation")
    ap.add_argument("--conv-valid", default="", help="convolutions with VALID padding: block;block")
    ap.add_argument("--blocks2d", default="", help="a 2-D convolutional graph instead of --blocks: out_channels,kh,kw,pool per block, e.g. \"8,3,3,2;16,3,3,2\"; "
                    "options after a colon, k=v pairs: stride=HxW valid=1 act=N bias=0 pool=HxW pool_stride=HxW pool_valid=1")
    ap.add_argument("--residual", default="", help="a residual graph instead of --blocks: steps name,conv,src,out_c,kh,kw,SHxSW,valid,act[,lift] | name,dw,src,depth_mult,kh,kw,SHxSW,valid,act[,lift] | name,add,a,b,act | "
                    "name,pool,src,PHxPW,SHxSW,valid[,keras], separated by ';' (src \"in\": the reshaped input), e.g. "
                    "\"c0,conv,in,16,1,3,1x1,0,1;m1,conv,c0,16,1,9,1x1,0,0;sum,add,c0,m1,1\"")
    ap.add_argument("--two-d", action="store_true", help="with --residual: the input is [1][frames][columns][1], not [1][1][frames][columns]")
    a = ap.parse_args()
    blocks = tuple(tuple(v if v in ("dw", "pw") else int(v) for v in b.split(",")) for b in a.blocks.split(";") if b)      # --blocks "": dense only
    dense = tuple(tuple(int(v) for v in d.split(",")) for d in a.dense.split(";") if d) or None
    def block2d(text):
        head, _, tail = text.partition(":")
        opt = {}
        for kv in tail.split():
            k, v = kv.split("=")
            opt[k] = tuple(int(x) for x in v.split("x")) if k in ("stride", "pool", "pool_stride") else bool(int(v)) if k in ("valid", "bias", "pool_valid") else int(v)
        return tuple(int(v) for v in head.split(",")) + ((opt,) if opt else ())
    blocks2d = tuple(block2d(b) for b in a.blocks2d.split(";") if b) or None

    def res_step(text):
        v = text.split(",")
        pair = lambda s: tuple(int(x) for x in s.split("x"))
        if v[1] in ("conv", "dw"):
            return (v[0], v[1], v[2], int(v[3]), int(v[4]), int(v[5]), pair(v[6]), bool(int(v[7])), int(v[8])) + ((float(v[9]),) if len(v) > 9 else ())
        if v[1] == "add":
            return (v[0], "add", v[2], v[3], int(v[4]))
        return (v[0], "pool", v[2], pair(v[3]), pair(v[4]), bool(int(v[5]))) + ((bool(int(v[6])),) if len(v) > 6 else ())
    residual = tuple(res_step(s_) for s_ in a.residual.split(";") if s_) or None
    blob = synth_model_blob(a.seed, blocks2d=blocks2d, residual=residual, two_d=a.two_d, ncep=a.ncep, win_size=a.win_size, low=a.low, high=a.high, blocks=blocks,
                            n_labels=a.labels, num_filters=a.num_filters, logit_std=a.logit_std, dense=dense,
                            conv_valid=tuple(int(v) for v in a.conv_valid.split(";") if v),
                            conv_stride={int(v.split(":")[0]): int(v.split(":")[1]) for v in a.conv_stride.split(";") if v} or None,
                            conv_dilation={int(v.split(":")[0]): int(v.split(":")[1]) for v in a.conv_dilation.split(";") if v} or None)
    with open(a.out, "wb") as f:
        f.write(blob)
    print(a.out, len(blob), "bytes")


if __name__ == "__main__":
    main()
