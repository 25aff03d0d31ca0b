"""Named graphs with strided and dilated temporal convolutions shared by tests/test_strided_graphs_host.py,
tests/test_gpu_strided_graphs.py and tools/make_golden_strided.py: each an int8 graph with a calibrated head (or calibrated hidden layers) and its float32
twin (tools/dequantize_model.py).  49 x 13 features and the shipped DSP block (tools/synth_model.py's defaults) unless a spec says otherwise, so that the
graphs can share a bank with the shipped shape."""
import functools
import os

import numpy as np

import dense_testlib as D
from kws_testlib import GOLDEN, f32_pick_blocking, synth_model_blob

GOLDEN_STRIDED = os.path.join(GOLDEN, "strided_graphs.npz")
N_INPUTS = 64            # inputs per graph: the oracle's feature matrices of 56 synth clips, then 8 uniform rows in [-3, 3]
N_SYNTH = 56
INPUT_SEED = 5151



def _lift(t, n):
    """As drawn, a block's ReLU parks more than half of its outputs on the bound (zero-mean pre-activations under a negative ADD constant) and a test on such
    a graph proves little.  Block by block, on 256 standardised random feature matrices (what cmvnw hands the network): the constant in front of every ReLU /
    ReLU6 -- the ADD's int8 operand, or the convolution's int32 bias -- is set per channel so that the float twin's pre-activation has mean 0.7 x its own
    deviation (about a quarter of the outputs below zero); a ReLU6 convolution's weight scales are first set so that the pre-activations' deviation is 1.5.
    Then the hidden layers (if any), the activation ranges and the head are calibrated again.  Draws nothing from the model's generator."""
    sm = D.synth_model
    x = np.random.default_rng(77).standard_normal((256, t[0]["dims"][1]))
    for idx, nd in enumerate(n):
        is_add, is_conv = nd["op"] == 2, nd["op"] in (1, 6)
        act = nd["p"][0] if is_add else nd["p"][3] if is_conv else 0
        if act not in (1, 3):
            continue
        a = sm.float_forward(t, n[:idx], 0, x)[nd["in"][0]]
        if is_add:
            pre = a.reshape(-1, a.shape[-1])
            c = 0.7 * pre.std(axis=0) - pre.mean(axis=0)
            tc = t[nd["in"][1]]
            tc["scale"] = [float(np.float32(max(np.abs(c).max(), 1e-6) / 127.0))]
            tc["data"] = np.clip(np.round(c / tc["scale"][0]), -127, 127).astype(np.int8).tobytes()
            continue
        tw, tb = t[nd["in"][1]], t[nd["in"][2]]
        in_scale = t[nd["in"][0]]["scale"][0]
        nd["p"][3] = 0                                      # the pre-activation: this node without its clamp and bias
        tb["data"] = bytes(len(tb["data"]))
        if act == 3:
            pre = sm.float_forward(t, [nd], nd["in"][0], a)[nd["out"][0]]
            tw["scale"] = [float(np.float32(s_ * 1.5 / pre.std())) for s_ in tw["scale"]]
        pre = sm.float_forward(t, [nd], nd["in"][0], a)[nd["out"][0]]
        pre = pre.reshape(-1, pre.shape[-1])
        nd["p"][3] = act
        tb["scale"] = [float(np.float32(in_scale) * np.float32(s_)) for s_ in tw["scale"]]
        tb["data"] = np.round((0.7 * pre.std(axis=0) - pre.mean(axis=0)) / np.float64(tb["scale"])).astype(np.int32).tobytes()
    fcs = [nd for nd in n if nd["op"] == 4]
    sm.calibrate_hidden(t, n, 0, fcs[:-1], x)
    sm.calibrate_head(t, n, 0, fcs[-1]["in"][1], fcs[-1]["in"][2], fcs[-1]["out"][0], 1.5, 0, x=x)


_C = dict(logit_std=1.5, edit=_lift)
_M40 = dict(num_filters=40, ncep=40, low=300, high=0)
STRIDED_SPECS = {
    # ---- strided convolutions
    "s2_k3": dict(_C, seed=601, blocks=((16, 3, 1), (8, 3, 5)), conv_stride={0: 2}),                         # 49 -> 25, pad left 1
    "s2_even": dict(_C, seed=602, blocks=((8, 2, 1), (16, 3, 1)), conv_valid=(0,), conv_stride={1: 2}),      # 49 -> 48 (VALID) -> 24: total padding 1, left 0
    "s3_k7_pool": dict(_C, seed=603, blocks=((16, 7, 2),), conv_stride={0: 3}),                              # 49 -> 17 -> 9 (ragged pool)
    "s2_valid": dict(_C, seed=604, blocks=((16, 4, 1),), conv_valid=(0,), conv_stride={0: 2}),               # 49 -> 23: trailing rows never read
    "s5_k2": dict(_C, seed=605, blocks=((16, 2, 1),), conv_stride={0: 5}),                                   # 49 -> 10: total padding -2, clamped to 0
    # ---- dilated convolutions
    "d2_k3": dict(_C, seed=611, blocks=((16, 3, 1), (8, 3, 7)), conv_dilation={0: 2}),
    "d4_wide": dict(_C, seed=612, blocks=((16, 3, 7), (8, 3, 1)), conv_dilation={1: 4}),                     # 7 rows, effective filter 9
    "d3_valid": dict(_C, seed=613, blocks=((16, 5, 1),), conv_valid=(0,), conv_dilation={0: 3}),             # 49 -> 37
    "s2_d2": dict(_C, seed=614, blocks=((16, 3, 1), (8, 3, 5)), conv_stride={0: 2}, conv_dilation={0: 2}),
    "dw_d2_valid": dict(_C, seed=615, blocks=(("dw", 2, 3, 1, 1), ("pw", 8, 1)), conv_valid=(0,), conv_dilation={0: 2}),      # 49 -> 45
    # ---- depthwise, pointwise and chains
    "dw_s2": dict(_C, seed=621, blocks=((16, 3, 1), ("dw", 1, 3, 1, 1), ("pw", 8, 1)), conv_stride={1: 2}),  # multiplier 1, 16 channels
    "dw_s2_m2": dict(_C, seed=622, blocks=(("dw", 2, 3, 1, 1), ("pw", 8, 1)), conv_stride={0: 2}),           # multiplier 2, 13 channels
    "dw_s3_k5_pool": dict(_C, seed=623, blocks=((16, 3, 1), ("dw", 1, 5, 2, 3)), conv_stride={1: 3}),        # 49 -> 17 -> 9, relu6
    "pw_s2": dict(_C, seed=624, blocks=((16, 3, 1), ("pw", 8, 1)), conv_stride={1: 2}),                      # strided shortcut
    "s2_chain": dict(_C, seed=625, blocks=((16, 3, 1), (16, 3, 1), (8, 3, 1)), conv_stride={0: 2, 1: 2, 2: 2}),   # 49 -> 25 -> 13 -> 7
    "w98_s2": dict(_C, seed=626, frame_stride=0.01, blocks=((16, 3, 1), (8, 3, 7)), conv_stride={0: 2}),     # 98 -> 49 un-pooled
    # ---- routing: block 1 (16 -> 32 channels, no pool) would be a matrix-core block at stride 1
    "mc_s2": dict(_C, seed=631, blocks=((16, 3, 2), (32, 3, 1)), conv_stride={1: 2}),
    "mc_d2": dict(_C, seed=632, blocks=((16, 3, 2), (32, 3, 1)), conv_dilation={1: 2}),
    "trunk_s2": dict(seed=633, edit=_lift, blocks=((16, 3, 1),), conv_stride={0: 2}, dense=((20, 1),)),                  # the trunk forms
    "c40_s2": dict(_C, seed=634, **_M40, blocks=((32, 3, 1), (8, 3, 5)), conv_stride={0: 2}),                  # in_cpad 48 -> 64, vec4 float reads
    # ---- float32 blockings the shapes above do not reach (BLOCKING_CLASSES)
    "fb_f2": dict(_C, seed=641, blocks=((16, 3, 2),), conv_stride={0: 2}),                                   # 25 x 16, pool 2: tb 2 fused
    "fb_f4": dict(_C, seed=642, blocks=((48, 3, -4),), conv_stride={0: 3}),                                  # 17 x 48, VALID pool 4: tb 4 fused
    "fb_tb7": dict(_C, seed=643, blocks=((30, 3, 7),), conv_dilation={0: 2}),                                # 49 x 30, pool 7: the shipped first block, dilated
    "fb_tb1": dict(_C, seed=644, blocks=((16, 3, 7), (10, 3, 7)), conv_dilation={1: 2}),                     # 7 rows x 10 channels
    "fb_dw8": dict(_C, seed=645, blocks=((20, 2, 1), ("dw", 1, 3, 1, 1)), conv_valid=(0,), conv_stride={1: 2}),      # depthwise 24 x 20: tb 8 free
    "fb_dw8f": dict(_C, seed=646, blocks=((20, 2, 1), ("dw", 1, 3, 8, 1)), conv_valid=(0,), conv_stride={1: 2}),     # ... pool 8: tb 8 fused
}
# the disagreement that keeps SAME-padded dilated depthwise refused: the reference pads it as if dilation were 1 (depthwise_conv.cc:489-492)
DW_D2_SAME = dict(_C, seed=651, blocks=(("dw", 1, 3, 1, 1), ("pw", 8, 1)), conv_dilation={0: 2})

E2E_SPECS = ("s2_k3", "d2_k3", "dw_s2", "trunk_s2")
WAVE_SPECS = ("d4_wide", "s2_even", "w98_s2")


@functools.lru_cache(maxsize=None)
def strided_blob(name):
    return synth_model_blob(**(DW_D2_SAME if name == "dw_d2_same" else STRIDED_SPECS[name]))


@functools.lru_cache(maxsize=None)
def strided_twin(name):
    return D.dequantize_model.dequantize(strided_blob(name))


@functools.lru_cache(maxsize=None)
def strided_features(name):
    """[N_INPUTS][features] float32: the oracle's feature matrices of synth clips, then uniform rows in [-3, 3]"""
    o = D._get_oracle()
    m = D.oracle_model(o, strided_blob(name))
    _, f, _ = m.run_batch(o.synth(INPUT_SEED, 0, N_SYNTH), want_features=True)
    r = np.random.default_rng(INPUT_SEED).uniform(-3.0, 3.0, (N_INPUTS - N_SYNTH, f.shape[1])).astype(np.float32)
    return np.ascontiguousarray(np.concatenate([f, r]), np.float32)


def conv_geometry(blob):
    """per CONV_2D / DEPTHWISE_CONV_2D node of a blob: dict(in_w, in_c, out_w, out_c, taps, stride, dilation, padding, depthwise) as the tensors state it"""
    tens, nodes, _, _, _ = D.eon_import.parse_blob(blob)
    out = []
    for nd in nodes:
        if nd["op"] in (1, 6):
            x, w, y = tens[nd["in"][0]]["dims"], tens[nd["in"][1]]["dims"], tens[nd["out"][0]]["dims"]
            out.append(dict(in_w=x[2], in_c=x[3], out_w=y[2], out_c=y[3], taps=w[2], stride=nd["p"][1], dilation=nd["p"][4], padding=nd["p"][0],
                            depthwise=nd["op"] == 6))
    return out


def is_strided(blob):
    return any(g["stride"] != 1 or g["dilation"] != 1 for g in conv_geometry(blob))


def block_clamp_bounds(blob):
    """{block output tensor id: (lo, hi)}: the int8 values the block's last clamp (ADD's ReLU, or the convolution's fused activation) can park an output on"""
    tens, nodes, _, _, _ = D.eon_import.parse_blob(blob)
    producers = {nd["out"][0]: nd for nd in nodes}
    out = {}
    for tid in D.block_outputs(blob):
        nd = producers[tid]
        while nd["op"] in (0, 3):                           # RESHAPE / MAX_POOL_2D keep the values
            nd = producers[nd["in"][0]]
        act = nd["p"][0] if nd["op"] == 2 else nd["p"][3]
        sc, zp = tens[nd["out"][0]]["scale"][0], tens[nd["out"][0]]["zero"][0]
        lo, hi = -128, 127
        if act == 1:
            lo = max(lo, zp)
        elif act == 3:
            lo, hi = max(lo, zp), min(hi, zp + int(round(6.0 / sc)))
        out[tid] = (lo, hi)
    return out


def check_not_vacuous(name, blob, taps, out_rows, f_rows):
    """over the N_INPUTS inputs every conv block output takes >= 16 distinct values with at most half of its entries on a clamp bound, and the graph gives
    >= 8 distinct score rows, int8 and float; AssertionError otherwise"""
    for tid, (lo, hi) in block_clamp_bounds(blob).items():
        v = taps[tid]
        assert len(np.unique(v)) >= 16, "%s: block output %d takes %d values" % (name, tid, len(np.unique(v)))
        assert np.mean((v <= lo) | (v >= hi)) <= 0.5, "%s: more than half of block output %d sits on a clamp bound" % (name, tid)
    assert len(np.unique(out_rows, axis=0)) >= 8 and len(np.unique(f_rows, axis=0)) >= 8, "%s: fewer than 8 distinct score rows" % name


def oracle_f32_blocks(oracle, blob, feats):
    """float twin: ({tensor id: [n][size] float32} for the block outputs, the hidden tensors and the logits, scores [n][labels])"""
    m = D.oracle_model(oracle, blob)
    _, _, hidden, last, _, _ = D.graph_layout(blob)
    taps = {i: [] for i in hidden + [last] + D.block_outputs(blob)}
    outs = []
    for row in feats:
        out, tp = m.nn_invoke_f32(row, taps=True)
        outs.append(out)
        for i in taps:
            taps[i].append(tp[i].copy())
    return {i: np.stack(v) for i, v in taps.items()}, np.stack(outs)


# ---- float32 blockings --------------------------------------------------------------------------------------------------------------------------
# Every (tb, fused) class kws_nn_f32_pick_blocking can return for a strided or dilated block: the pick depends on the block's OUTPUT shape only (out_w,
# out_c, pool), which stride and dilation change but do not constrain, so the classes are the ones of the stride-1 table: tb 1, 2, 4, 7, 8 free (direct or
# staged), and fused tb = pool for the pools that fuse (2, 4, 7, 8).  tb = 1 cannot be fused (a pool of 1 is no pooling node).
BLOCKING_CLASSES = {(1, False), (2, False), (4, False), (7, False), (8, False), (2, True), (4, True), (7, True), (8, True)}


def f32_blockings(blob):
    """[(tb, fused, strided)] per conv block of a float graph by the restated pick (kws_testlib.f32_pick_blocking; the GPU test asserts the library's own)"""
    tens, nodes, _, _, _ = D.eon_import.parse_blob(blob)
    out = []
    for k, nd in enumerate(nodes):
        if nd["op"] not in (1, 6):
            continue
        y = tens[nd["out"][0]]["dims"]
        out_w, out_c, pool, pstride, pool_w = y[2], y[3], 1, 1, y[2]
        for nx in nodes[k + 1:]:
            if nx["op"] in (1, 6, 4):
                break
            if nx["op"] == 3:
                pool, pstride, pool_w = nx["p"][4], nx["p"][2], tens[nx["out"][0]]["dims"][1]
        tb, ob, mode = f32_pick_blocking(nd["op"] == 6, out_w, out_c, pool, pstride, pool_w)
        out.append((tb, mode == "fused", nd["p"][1] != 1 or nd["p"][4] != 1))
    return out
