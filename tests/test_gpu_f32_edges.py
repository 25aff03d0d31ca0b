"""-m gpu: the float32 network kernels (kws_nn_f32_kernel<512> / <1024>, its trunk form, kws_dense_f32_kernel) over every blocking
kws_nn_f32_pick_blocking can choose (kws_testlib.F32_BLOCKINGS -- the plan's pick is asserted through kws_dev_f32_blocking) and at float
edges (kws_testlib.F32_EDGES: every fused activation on every op, subnormals, signed zeros, overflow, softmax), through the network-only
entry point: logits bit for bit (NaN for NaN) against the restatement on every input row and against the reference's recorded results
(tests/golden/f32_edges_l476.npz) on the first 4, scores within F32_SCORE_TOL with the same NaN mask.  The CPU pins
(tests/test_oracle_vs_reference.py, tests/test_oracle_golden.py) hold the restatement to the reference on the same graphs and inputs and
assert that each case tests something."""
import ctypes

import numpy as np
import pytest

from kws_testlib import (F32_BLOCKINGS, F32_EDGES, F32_GOLDEN_ROWS, F32_MULTIPASS, F32_REFUSALS, ROOT, OracleModel, bits, f32_blob,
                         f32_blocking_name, f32_case_inputs, f32_edge_groups, f32_golden, f32_graph_blocks, f32_inputs, f32_launch_shape,
                         f32_prefetch_eligible, same_bits_or_both_nan, synth_model_blob)

pytestmark = pytest.mark.gpu

F32_SCORE_TOL = 1e-6           # the project's bar for exact-mode float32 scores (the float softmax uses the device expf, kws.h)


@pytest.fixture(scope="module")
def pkg():
    import sys
    sys.path.insert(0, ROOT)
    import torch  # noqa: F401  (first: libamdhip64 of the torch wheel is the one the process uses)
    from __graft_entry__ import load_package
    return load_package()


@pytest.fixture(scope="module")
def golden():
    return f32_golden()


def run_network(gm, feats):
    import torch
    f = torch.from_numpy(np.ascontiguousarray(feats, np.float32)).to("cuda:0")
    B = f.shape[0]
    s = torch.empty((B, gm.n_labels), dtype=torch.float32, device="cuda:0")
    lg = torch.empty((B, gm.n_labels), dtype=torch.float32, device="cuda:0")
    gm.nn_f32_batch_device(f.data_ptr(), B, s.data_ptr(), lg.data_ptr())
    torch.cuda.synchronize()
    return s.cpu().numpy(), lg.cpu().numpy()


def plan_blocking(pkg, gm, block):
    """kws_dev_f32_blocking -> (return code, dict in the keys of kws_testlib.f32_graph_blocks + waves, smem)"""
    L = pkg.lib()
    L.kws_dev_f32_blocking.restype = ctypes.c_int
    L.kws_dev_f32_blocking.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(ctypes.c_int * 8)]
    out = (ctypes.c_int * 8)(*([-77] * 8))
    rc = L.kws_dev_f32_blocking(gm.h, block, ctypes.byref(out))
    tb, ob, fused, ntb, rows, dw, waves, smem = list(out)
    return rc, dict(tb=tb, ob=ob, fused=fused, ntb=ntb, rows=rows, depthwise=bool(dw), waves=waves, smem=smem), list(out)


def check_graph(pkg, oracle, tmp_path, key, entry, golden):
    """one table graph: the plan's choices against the restated ones (and the entry's name, for a blocking entry), then the library's logits
    and scores over the entry's input rows against the restatement's and the recorded reference's.  Returns the open model."""
    blob = f32_blob(entry)
    p = tmp_path / "m.kwsm"
    p.write_bytes(blob)
    om = OracleModel(oracle, str(p))
    gm = pkg.Model(blob=blob)
    blocks, _ = f32_graph_blocks(blob)
    waves, smem = f32_launch_shape(blob)
    for b, want in enumerate(blocks):
        rc, got, _ = plan_blocking(pkg, gm, b)
        assert rc == 0, (key, b, rc)
        got["mode"] = "fused" if got["fused"] else "direct" if want["pool"] == 1 else "staged"
        assert f32_blocking_name(got) == f32_blocking_name(want), (key, b, got)
        assert (got["ntb"], got["rows"], got["waves"], got["smem"]) == (want["ntb"], want["rows"], waves, smem), (key, b, got, want["ntb"], want["rows"], waves, smem)
        if "block" in entry and b == entry["block"]:
            assert f32_blocking_name(got) == key.split("/", 1)[1].split("#")[0], (key, got)        # the blocking the table names
    xs = f32_case_inputs(entry, om.n_features)
    s, lg = run_network(gm, xs)
    n_t = len(om.tensor_bytes)
    bad = []
    for i, x in enumerate(xs):
        so, taps = om.nn_invoke_f32(x, taps=True)
        if not same_bits_or_both_nan(lg[i], taps[n_t - 2]):
            bad.append((i, "logits", lg[i].tolist(), np.asarray(taps[n_t - 2]).tolist()))
        elif not ((np.isnan(s[i]) == np.isnan(so)).all() and np.abs(np.nan_to_num(s[i] - so)).max() <= F32_SCORE_TOL):
            bad.append((i, "scores", s[i].tolist(), so.tolist()))
    assert not bad, (key, len(bad), bad[:3])
    g = golden[key]
    assert same_bits_or_both_nan(lg[:F32_GOLDEN_ROWS], g["logits"]), key
    assert (np.isnan(s[:F32_GOLDEN_ROWS]) == np.isnan(g["scores"])).all(), key
    assert np.abs(np.nan_to_num(s[:F32_GOLDEN_ROWS] - g["scores"])).max() <= F32_SCORE_TOL, key
    return gm


@pytest.mark.parametrize("group", sorted({k.rsplit("/", 2)[0] for k in F32_BLOCKINGS}))
def test_f32_network_at_every_blocking(group, pkg, oracle, golden, tmp_path):
    """Every entry of F32_BLOCKINGS of one kind (CONV_2D / DEPTHWISE_CONV_2D) and tb: the plan picked the (tb, ob, output mode) the entry
    names -- a change to the cost model fails here instead of quietly shrinking coverage --, ntb / rows / waves / LDS bytes are the restated
    ones, and logits and scores are the restatement's over all input rows."""
    keys = [k for k in F32_BLOCKINGS if k.rsplit("/", 2)[0] == group]
    assert keys
    for key in keys:
        check_graph(pkg, oracle, tmp_path, "blocking/" + key, F32_BLOCKINGS[key], golden).close()


@pytest.mark.parametrize("group", f32_edge_groups())
def test_f32_network_at_float_edges(group, pkg, oracle, golden, tmp_path):
    """Every case of one family of F32_EDGES: one op's four fused activations with pre-activations exactly on and one ulp beside the clamp
    bounds, subnormal block-0 activations, signed-zero inputs and constants (the sign of a zero logit included), products that overflow,
    softmax at other beta / logits 200 apart / equal logits / 2, 47 and 48 labels."""
    keys = [k for k in F32_EDGES if k.split("/")[0] == group]
    assert keys
    for key in keys:
        check_graph(pkg, oracle, tmp_path, "edge/" + key, F32_EDGES[key], golden).close()


@pytest.mark.parametrize("key", sorted(F32_REFUSALS))
def test_float_models_kws_create_must_refuse(key, pkg):
    """49 labels, 17 taps, 65 output channels, a pool window of 9, nine conv blocks, weights past the LDS budget; and a non-finite conv /
    depthwise / FULLY_CONNECTED weight (0 * inf = NaN on a zero-padded row where the reference skips the tap): KWS_ERROR_UNSUPPORTED_MODEL
    from kws_create, the message naming the tensor of a non-finite weight."""
    r = F32_REFUSALS[key]
    with pytest.raises(pkg.KwsError) as ei:
        pkg.Model(blob=f32_blob(r))
    assert ei.value.code == -18, (key, str(ei.value))
    assert r["says"] in str(ei.value), (key, str(ei.value))
    if key.startswith("non_finite/"):
        assert "tensor" in str(ei.value), str(ei.value)


def test_blocking_accessor_refuses_what_it_cannot_answer(pkg):
    """kws_dev_f32_blocking: a negative value and an untouched out[] for an int8 handle and for a block index outside 0 .. n_blocks - 1"""
    kw = F32_MULTIPASS["b1024"][0]
    gi = pkg.Model(blob=synth_model_blob(**kw))
    rc, _, raw = plan_blocking(pkg, gi, 0)
    assert rc < 0 and raw == [-77] * 8
    gi.close()
    gf = pkg.Model(blob=f32_blob(dict(kw=kw)))
    assert plan_blocking(pkg, gf, 0)[0] == 0 and plan_blocking(pkg, gf, 1)[0] == 0
    for b in (-1, 2, 8):
        rc, _, raw = plan_blocking(pkg, gf, b)
        assert rc < 0 and raw == [-77] * 8, b
    gf.close()


@pytest.mark.parametrize("key", sorted(F32_MULTIPASS))
def test_second_and_later_clips_per_wave(key, pkg, oracle, tmp_path):
    """A batch of 2 x resident + 37 clips (resident = CUs x workgroups per CU x waves: what the grid holds before a wave loops), so every wave
    serves a second and a third clip: the next-clip prefetch, the re-zeroed padding rows and the reuse of a wave's LDS images between clips.
    The rows repeat 64 base rows in a shuffled order: each must equal its base row's output bit for bit, and the 64 base rows equal the
    restatement.  One handle per kernel form: <512> with the prefetch eligible and not, <1024>, and a dense stack behind the trunk form."""
    import torch
    kw, want = F32_MULTIPASS[key]
    blob = f32_blob(dict(kw=kw))
    p = tmp_path / "m.kwsm"
    p.write_bytes(blob)
    om = OracleModel(oracle, str(p))
    gm = pkg.Model(blob=blob)
    rc, got, _ = plan_blocking(pkg, gm, 0)
    assert rc == 0 and (got["waves"], got["smem"]) == f32_launch_shape(blob), (key, got)
    assert got["waves"] <= want.get("waves_max", 16) and got["waves"] >= want.get("waves_min", 1), (key, got)
    assert f32_prefetch_eligible(blob) == want["prefetch"], key
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    resident = n_cu * max(1, (160 * 1024) // got["smem"]) * got["waves"]
    assert resident <= 16 * 1024 + 4096, (key, resident)
    base = f32_inputs(om.n_features, 64, seed=477)
    sb, lb = run_network(gm, base)
    n_t = len(om.tensor_bytes)
    for i in range(64):
        so, taps = om.nn_invoke_f32(base[i], taps=True)
        assert (bits(lb[i]) == bits(taps[n_t - 2])).all(), (key, i)
        assert np.abs(sb[i] - so).max() <= F32_SCORE_TOL, (key, i)
    B = 2 * resident + 37
    idx = np.random.default_rng(478).integers(0, 64, B)
    s, lg = run_network(gm, base[idx])
    wrong = np.nonzero((bits(lg) != bits(lb[idx])).any(axis=1) | (bits(s) != bits(sb[idx])).any(axis=1))[0]
    assert wrong.size == 0, (key, B, resident, wrong.size, wrong[:8].tolist())
    gm.close()
