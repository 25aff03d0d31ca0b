"""-m gpu: graphs with DEPTHWISE_CONV_2D steps on the step trunks through the C ABI, against the oracle (pinned to the reference by
tests/golden/dwres_graphs.npz, tests/test_dwres_graphs_host.py): the step trunk + dense kernels alone (every step output, bit for bit), batches in which
every wave serves several clips, the batch call and the SDK from PCM, the fast-mode refusal on a graph without an ADD, the refusals' messages, and the
kernels of the graphs served before."""
import ctypes
import os
import sys

import numpy as np
import pytest

import dense_testlib as D
import dwres_testlib as T
from kws_testlib import MODELS, ROOT, bits
from test_dwres_graphs_host import _bias_minus_one

pytestmark = pytest.mark.gpu

F32_SCORE_TOL = 1e-6           # the project's bar for exact-mode float32 scores (the float softmax uses the device expf)
NAMES = list(T.DW_SPECS)
KERNEL_I8 = "kws_nnres_trunk_kernel + kws_dense_i8_kernel"
KERNEL_F32 = "kws_nnres_f32_trunk_kernel + kws_dense_f32_kernel"


@pytest.fixture(scope="module")
def pkg():
    sys.path.insert(0, ROOT)
    import torch  # noqa: F401
    from __graft_entry__ import load_package
    return load_package()


@pytest.fixture(scope="module")
def gpu_models(pkg):
    made = {}

    def get(name, twin=False):
        key = (name, twin)
        if key not in made:
            if name.endswith(".kwsm"):
                made[key] = pkg.Model(os.path.join(MODELS, name))
            else:
                made[key] = pkg.Model(blob=T.dw_twin(name) if twin else T.dw_blob(name))
        return made[key]

    yield get
    for m in made.values():
        m.close()


@pytest.fixture(scope="module")
def expected(oracle):
    """per graph: the oracle's tensors on res_features() (int8) / res_twin_features() (twin), computed once"""
    made = {}

    def get(name, twin=False):
        key = (name, twin)
        if key not in made:
            made[key] = (T.oracle_f32(oracle, T.dw_twin(name), T.res_twin_features()) if twin else T.oracle_int8(oracle, T.dw_blob(name), T.res_features()))
        return made[key]

    return get


@pytest.fixture(scope="module")
def fixture_npz():
    return np.load(T.GOLDEN_DWRES)


def run_f32(gm, x):
    """kws_nn_f32_batch_device with a sentinel row behind the batch: nothing behind the batch is written"""
    import torch
    B = x.shape[0]
    d_f = torch.from_numpy(np.array(x, np.float32)).cuda()
    d_s = torch.full((B + 1, gm.n_labels), -7.0, dtype=torch.float32, device="cuda")
    d_l = torch.full((B + 1, gm.n_labels), -7.0, dtype=torch.float32, device="cuda")
    gm.nn_f32_batch_device(d_f.data_ptr(), B, d_s.data_ptr(), d_l.data_ptr())
    torch.cuda.synchronize()
    s, lg = d_s.cpu().numpy(), d_l.cpu().numpy()
    assert np.all(s[B] == -7.0) and np.all(lg[B] == -7.0)
    return s[:B], lg[:B]


def score_error(s, want):
    """max |s - want| over the finite entries; a NaN must sit where the oracle's sits"""
    assert np.array_equal(np.isnan(s), np.isnan(want))
    ok = ~np.isnan(want)
    return float(np.abs(s[ok] - want[ok]).max()) if ok.any() else 0.0


def check_int8_taps(name, gm, blob, q, taps, out_q, scores):
    """kws_nn_batch_device with every tap against the oracle's tensors, tensor by tensor so that a failure names the step"""
    _, _, hidden, last, _, _ = D.graph_layout(blob)
    ids = T.step_outputs(blob) + hidden
    assert gm.pooled_tap_bytes == sum(taps[i].shape[1] for i in ids)
    s, tp, tf, to = gm.nn_batch(q)
    at = 0
    for b, i in enumerate(ids):
        assert np.array_equal(tp[:, at:at + taps[i].shape[1]], taps[i]), (name, "step / hidden tensor", b)
        at += taps[i].shape[1]
    assert np.array_equal(tf, taps[last]) and np.array_equal(to, out_q), name
    assert np.array_equal(bits(s), bits(scores)), name


@pytest.mark.parametrize("name", NAMES)
def test_network_int8_every_step_output(name, gpu_models, expected, fixture_npz):
    """kws_nn_batch_device with every tap: each step's (pooled) output, hidden tensors, tap_fc, tap_out and scores, bit for bit, every input"""
    gm = gpu_models(name)
    q, taps, out_q, scores = expected(name)
    assert np.array_equal(out_q, fixture_npz[name + "/scores"])              # the oracle is the reference's here too
    assert gm.nn_kernel == KERNEL_I8, gm.nn_kernel
    assert gm.depthwise_step_count == T.N_DW[name] and gm.residual_add_count == T.N_ADDS[name] and gm.conv2d_block_count == 0 and not gm.is_float
    check_int8_taps(name, gm, T.dw_blob(name), q, taps, out_q, scores)


@pytest.mark.parametrize("name", NAMES)
def test_network_float32(name, gpu_models, expected, fixture_npz):
    """kws_nn_f32_batch_device on the twin: logits bit for bit (NaN by position), scores within 1e-6 of the oracle"""
    gm = gpu_models(name, twin=True)
    ftaps, fscores = expected(name, twin=True)
    assert T.same_bits_nan_by_position(fscores, fixture_npz[name + "/fscores"].view(np.float32))
    assert gm.is_float and gm.nn_kernel == KERNEL_F32, gm.nn_kernel
    assert gm.depthwise_step_count == T.N_DW[name] and gm.residual_add_count == T.N_ADDS[name] and gm.conv2d_block_count == 0
    _, _, _, last, _, _ = D.graph_layout(T.dw_blob(name))
    s, lg = run_f32(gm, T.res_twin_features())
    assert T.same_bits_nan_by_position(lg, ftaps[last]), name
    err = score_error(s, fscores)
    print(name, "max |score - oracle| = %.3g" % err)
    assert err <= F32_SCORE_TOL, name


def test_no_bias_as_a_minus_one_input(pkg, gpu_models, expected):
    """dw_no_bias with the depthwise node's bias spelled in[2] = -1 (three inputs) instead of two inputs: the same tensors and scores, int8 and float"""
    q, taps, out_q, scores = expected("dw_no_bias")
    blob = _bias_minus_one(T.dw_blob("dw_no_bias"))
    gm = pkg.Model(blob=blob)
    try:
        assert gm.depthwise_step_count == 1
        check_int8_taps("dw_no_bias (in[2] = -1)", gm, blob, q, taps, out_q, scores)
    finally:
        gm.close()
    gm = pkg.Model(blob=_bias_minus_one(T.dw_twin("dw_no_bias")))
    try:
        s, lg = run_f32(gm, T.res_twin_features())
        s0, lg0 = run_f32(gpu_models("dw_no_bias", True), T.res_twin_features())
        assert T.same_bits_nan_by_position(lg, lg0) and T.same_bits_nan_by_position(s, s0)
    finally:
        gm.close()


@pytest.mark.parametrize("twin", (False, True), ids=("int8", "f32"))
@pytest.mark.parametrize("name", T.MULTI_CLIP_SPECS)
def test_second_and_later_clips_per_wave(name, twin, gpu_models, expected):
    """a batch of 2 x resident + 37 inputs (resident: what the grid holds before a wave loops -- one workgroup of at most 16 waves per CU), so every wave
    serves a second and a third clip and every slot is reused: padding or values a previous clip or step left behind would show here.  The rows repeat the
    reference inputs in a shuffled order; EVERY clip is compared with the oracle's output for its row.  Nothing behind the batch is written."""
    import torch
    gm = gpu_models(name, twin)
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    resident = n_cu * 16
    assert resident <= 16 * 1024, resident
    B = 2 * resident + 37
    blob = T.dw_blob(name)
    _, _, _, last, _, _ = D.graph_layout(blob)
    if twin:
        ftaps, fscores = expected(name, True)
        idx = np.random.default_rng(481).integers(0, T.N_STD + T.N_FLOAT, B)
        s, lg = run_f32(gm, T.res_twin_features()[idx])
        same = ((bits(lg) == bits(ftaps[last][idx])) | (np.isnan(lg) & np.isnan(ftaps[last][idx]))).all(axis=1)
        close = (np.isnan(s) == np.isnan(fscores[idx])).all(axis=1) & ~(np.abs(s - fscores[idx]) > F32_SCORE_TOL).any(axis=1)
        wrong = np.nonzero(~(same & close))[0]
    else:
        q, taps, out_q, scores = expected(name)
        idx = np.random.default_rng(481).integers(0, T.N_STD, B)
        d_q = torch.from_numpy(np.ascontiguousarray(q[idx])).cuda()
        d_s = torch.full((B + 1, gm.n_labels), -7.0, dtype=torch.float32, device="cuda")
        gm.nn_batch_device(d_q.data_ptr(), B, d_s.data_ptr())
        torch.cuda.synchronize()
        s = d_s.cpu().numpy()
        assert np.all(s[B] == -7.0)
        s2, tp, tf, to = gm.nn_batch(q[idx])
        want = np.concatenate([taps[i] for i in T.step_outputs(blob)], axis=1)
        wrong = np.nonzero((tp != want[idx]).any(axis=1) | (to != out_q[idx]).any(axis=1) | (bits(s[:B]) != bits(scores[idx])).any(axis=1) |
                           (bits(s2) != bits(scores[idx])).any(axis=1))[0]
    assert wrong.size == 0, (name, B, resident, wrong.size, wrong[:8].tolist())


# ---- from PCM ------------------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def clips(oracle):
    pcm = oracle.synth(81, 0, 32)
    pcm.setflags(write=False)
    return pcm


@pytest.mark.parametrize("twin", (False, True), ids=("int8", "f32"))
@pytest.mark.parametrize("name", T.E2E_SPECS)
def test_batch_call_and_sdk_from_pcm(name, twin, pkg, gpu_models, oracle, clips):
    """kws_run_classifier_batch_device on 32 synth clips (features, the int8 input tensor, scores against OracleModel.run_batch), then the SDK's
    run_classifier on one of them against the oracle"""
    import torch
    gm = gpu_models(name, twin)
    om = D.oracle_model(oracle, T.dw_twin(name) if twin else T.dw_blob(name))
    es, ef, eq = om.run_batch(clips, want_features=True)
    B = clips.shape[0]
    d_pcm = torch.from_numpy(np.ascontiguousarray(clips)).cuda()
    d_s = torch.empty((B, gm.n_labels), dtype=torch.float32, device="cuda")
    d_f = torch.empty((B, gm.n_features), dtype=torch.float32, device="cuda")
    d_q = torch.empty((B, gm.n_features), dtype=torch.int8, device="cuda")
    gm.run_classifier_batch_device(d_pcm.data_ptr(), B, d_s.data_ptr(), d_f.data_ptr(), None if twin else d_q.data_ptr())
    torch.cuda.synchronize()
    s, f = d_s.cpu().numpy(), d_f.cpu().numpy()
    assert np.array_equal(bits(f), bits(ef))
    if twin:
        print(name, "batch max |score - oracle| = %.3g" % float(np.abs(s - es).max()))
        assert np.abs(s - es).max() <= F32_SCORE_TOL
    else:
        assert np.array_equal(d_q.cpu().numpy(), eq)
        assert np.array_equal(bits(s), bits(es))
    gm.set_default()
    try:
        buf = clips[5].astype(np.float32) / np.float32(32768)

        @pkg.GET_DATA_FN
        def get_data(offset, length, out):
            ctypes.memmove(out, buf[offset:offset + length].ctypes.data, 4 * length)
            return 0
        sig = pkg.Signal(get_data=get_data, total_length=16000)
        res = pkg.result_struct(gm.n_labels)()
        assert pkg.lib().run_classifier(ctypes.byref(sig), ctypes.byref(res), False) == 0
        got = np.float32([res.classification[i].value for i in range(gm.n_labels)])
        want = om.run_batch(clips[5:6])[0]
        assert np.abs(got - want).max() <= F32_SCORE_TOL if twin else np.array_equal(bits(got), bits(want))
    finally:
        gpu_models("l476_no_yes.kwsm").set_default()


@pytest.mark.parametrize("twin", (True, False), ids=("f32", "int8"))
def test_fast_mode_is_refused_without_an_add(twin, pkg, oracle, clips):
    """kws_set_mode(KWS_MODE_FAST) on ds2d_plain (no ADD): KWS_ERROR_UNSUPPORTED_MODEL with a message that names the family, and the handle goes on
    serving KWS_MODE_EXACT"""
    import torch
    blob = T.dw_twin("ds2d_plain") if twin else T.dw_blob("ds2d_plain")
    gm = pkg.Model(blob=blob)
    try:
        assert gm.residual_add_count == 0 and gm.depthwise_step_count == 1
        with pytest.raises(pkg.KwsError) as ei:
            gm.set_mode(pkg.MODE_FAST)
        assert ei.value.code == -18 and "depthwise" in str(ei.value) and "exact kernels" in str(ei.value)
        es = D.oracle_model(oracle, blob).run_batch(clips[:16])
        d_pcm = torch.from_numpy(np.ascontiguousarray(clips[:16])).cuda()
        d_s = torch.empty((16, gm.n_labels), dtype=torch.float32, device="cuda")
        gm.run_classifier_batch_device(d_pcm.data_ptr(), 16, d_s.data_ptr())
        torch.cuda.synchronize()
        s = d_s.cpu().numpy()
        assert np.abs(s - es).max() <= F32_SCORE_TOL if twin else np.array_equal(bits(s), bits(es))
    finally:
        gm.close()


def test_fast_mode_wording_with_an_add_is_unchanged(pkg):
    """a graph with an ADD and depthwise steps (mbx_block) keeps the residual wording of DESIGN 4.17"""
    gm = pkg.Model(blob=T.dw_blob("mbx_block"))
    try:
        with pytest.raises(pkg.KwsError) as ei:
            gm.set_mode(pkg.MODE_FAST)
        assert ei.value.code == -18 and "fast mode: a residual graph keeps the exact kernels (no fused plan, no calibrated logit gain)" in str(ei.value)
    finally:
        gm.close()


def test_refusal_messages(pkg):
    """what DESIGN 4.18 leaves out: -18 from kws_create, the message naming the node as "conv N:", DEPTHWISE_CONV_2D and the reason"""
    blobs = T.refused_blobs()
    assert blobs
    for key, (_, which, says) in T.REFUSED.items():
        for k in [key] * (which in ("both", "int8")) + [key + "_f32"] * (which in ("both", "f32")):
            with pytest.raises(pkg.KwsError) as ei:
                pkg.Model(blob=blobs[k])
            msg = str(ei.value)
            assert ei.value.code == -18 and all(w in msg for w in says), (k, msg)


def test_graphs_served_before_keep_their_kernels(pkg):
    """kws_depthwise_step_count is 0 and kws_nn_kernel_name unchanged for the shipped models, the 1-D depthwise chain dscnn_a (block kernels), one strided
    depthwise graph, one 2-D graph and one residual graph served before"""
    from test_gpu_strided_graphs import PARENT_KERNELS
    import conv2d_testlib as C2
    import dequantize_model
    import residual_testlib as R
    import strided_testlib as S
    from kws_testlib import SYNTH_SPECS, synth_model_blob
    got = {}
    for fn in sorted(os.listdir(MODELS)):
        if fn.endswith(".kwsm"):
            gm = pkg.Model(os.path.join(MODELS, fn))
            got["m_" + fn[:-5]] = (gm.nn_kernel, gm.depthwise_step_count, gm.residual_add_count)
            gm.close()
    blob = synth_model_blob(**SYNTH_SPECS["dscnn_a"])
    for suffix, b in (("", blob), ("_f32", dequantize_model.dequantize(blob))):
        gm = pkg.Model(blob=b)
        got["s_dscnn_a" + suffix] = (gm.nn_kernel, gm.depthwise_step_count, gm.residual_add_count)
        gm.close()
    assert got == {k: (PARENT_KERNELS[k], 0, 0) for k in got}, got
    for blob, want, adds in ((S.strided_blob("dw_s2"), "kws_nn_sd_kernel", 0), (S.strided_twin("dw_s2"), "kws_nn_f32_sd_kernel", 0),
                             (C2.conv2d_blob("ei_2d"), "kws_nn2d_trunk_kernel + kws_dense_i8_kernel", 0),
                             (C2.conv2d_twin("ei_2d"), "kws_nn2d_f32_trunk_kernel + kws_dense_f32_kernel", 0),
                             (R.res_blob("tc_proj_s2"), KERNEL_I8, 1), (R.res_twin("res2d_identity"), KERNEL_F32, 1)):
        gm = pkg.Model(blob=blob)
        assert (gm.nn_kernel, gm.depthwise_step_count, gm.residual_add_count) == (want, 0, adds)
        gm.close()
