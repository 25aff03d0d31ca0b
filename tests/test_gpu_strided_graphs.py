"""-m gpu: strided and dilated temporal convolutions through the C ABI, against the oracle (pinned to the reference by
tests/golden/strided_graphs.npz, tests/test_strided_graphs_host.py): the strided forms of the generic kernels alone (every block output, bit for bit),
the batch call from PCM, batches in which every wave serves several clips, the SDK entry points, a bank, a ragged call, a slide, the fast-mode refusal,
the refusals' messages, and the kernels of the graphs served before."""
import ctypes
import os
import sys

import numpy as np
import pytest

import dense_testlib as D
import strided_testlib as S
from kws_testlib import MODELS, ROOT, SYNTH_SPECS, bits, synth_model_blob

pytestmark = pytest.mark.gpu

F32_SCORE_TOL = 1e-6           # the project's bar for exact-mode float32 scores (the float softmax uses the device expf)
NAMES = list(S.STRIDED_SPECS)
SD_NAMES_I8 = ("kws_nn_sd_kernel", "kws_nn_sd_trunk_kernel + kws_dense_i8_kernel")
SD_NAMES_F32 = ("kws_nn_f32_sd_kernel", "kws_nn_f32_sd_trunk_kernel + kws_dense_f32_kernel")


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
                made[key] = pkg.Model(blob=S.strided_twin(name) if twin else S.strided_blob(name))
        return made[key]

    yield get
    for m in made.values():
        m.close()


@pytest.fixture(scope="module")
def expected(oracle):
    """per graph: the oracle's tensors on strided_features(), computed once"""
    made = {}

    def get(name, twin=False):
        key = (name, twin)
        if key not in made:
            f = S.strided_features(name)
            made[key] = S.oracle_f32_blocks(oracle, S.strided_twin(name), f) if twin else D.oracle_int8(oracle, S.strided_blob(name), f)
        return made[key]

    return get


@pytest.fixture(scope="module")
def fixture_npz():
    return np.load(S.GOLDEN_STRIDED)


def run_f32(gm, x):
    import torch
    B = x.shape[0]
    d_f = torch.from_numpy(np.ascontiguousarray(x, np.float32)).cuda()
    d_s = torch.full((B + 1, gm.n_labels), -7.0, dtype=torch.float32, device="cuda")
    d_l = torch.full((B + 1, gm.n_labels), -7.0, dtype=torch.float32, device="cuda")
    gm.nn_f32_batch_device(d_f.data_ptr(), B, d_s.data_ptr(), d_l.data_ptr())
    torch.cuda.synchronize()
    s, lg = d_s.cpu().numpy(), d_l.cpu().numpy()
    assert np.all(s[B] == -7.0) and np.all(lg[B] == -7.0)                 # nothing behind the batch is written
    return s[:B], lg[:B]


def plan_blocking(pkg, gm, block):
    """kws_dev_f32_blocking -> dict(tb, ob, fused, ntb, rows, depthwise, waves, smem) of a float handle's conv block"""
    L = pkg.lib()
    L.kws_dev_f32_blocking.restype = ctypes.c_int
    L.kws_dev_f32_blocking.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(ctypes.c_int * 8)]
    out = (ctypes.c_int * 8)(*([-77] * 8))
    assert L.kws_dev_f32_blocking(gm.h, block, ctypes.byref(out)) == 0
    return dict(zip(("tb", "ob", "fused", "ntb", "rows", "depthwise", "waves", "smem"), list(out)))


@pytest.mark.parametrize("name", NAMES)
def test_network_int8_every_block_output(name, gpu_models, expected, fixture_npz):
    """kws_nn_batch_device with every tap: each block's (pooled) output, hidden tensors, tap_fc, tap_out and scores, bit for bit, every input"""
    gm = gpu_models(name)
    q, taps, out_q, scores = expected(name)
    assert np.array_equal(out_q, fixture_npz[name + "/scores"])              # the oracle is the reference's here too
    assert gm.nn_kernel in SD_NAMES_I8, gm.nn_kernel
    _, _, hidden, last, _, _ = D.graph_layout(S.strided_blob(name))
    want = np.concatenate([taps[i] for i in D.block_outputs(S.strided_blob(name)) + hidden], axis=1)
    assert gm.pooled_tap_bytes == want.shape[1]
    s, tp, tf, to = gm.nn_batch(q)
    assert np.array_equal(tp, want), name
    assert np.array_equal(tf, taps[last]) and np.array_equal(to, out_q), name
    assert np.array_equal(bits(s), bits(scores)), name


@pytest.mark.parametrize("name", NAMES)
def test_network_float32(name, pkg, gpu_models, expected, fixture_npz):
    """kws_nn_f32_batch_device on the twin: logits bit for bit, scores within 1e-6; the plan's blocking of every block is the restated one"""
    gm = gpu_models(name, twin=True)
    ftaps, fscores = expected(name, twin=True)
    assert np.array_equal(bits(fscores), bits(fixture_npz[name + "/fscores"]))
    assert gm.is_float and gm.nn_kernel in SD_NAMES_F32, gm.nn_kernel
    _, _, _, last, _, _ = D.graph_layout(S.strided_blob(name))
    for b, (tb, fused, _) in enumerate(S.f32_blockings(S.strided_twin(name))):
        got = plan_blocking(pkg, gm, b)
        assert (got["tb"], bool(got["fused"])) == (tb, fused), (name, b, got)
    s, lg = run_f32(gm, S.strided_features(name))
    assert np.array_equal(bits(lg), bits(ftaps[last])), name
    print(name, "max |score - oracle| = %.3g" % float(np.abs(s - fscores).max()))
    assert np.abs(s - fscores).max() <= F32_SCORE_TOL, name


def test_float_blocking_classes_are_covered(pkg, gpu_models):
    """every (tb, fused) class kws_nn_f32_pick_blocking can return is hit by a strided or dilated block of some twin: the library's own picks"""
    got = set()
    for name in NAMES:
        gm = gpu_models(name, twin=True)
        for b, g in enumerate(S.conv_geometry(S.strided_twin(name))):
            if g["stride"] != 1 or g["dilation"] != 1:
                pb = plan_blocking(pkg, gm, b)
                got.add((pb["tb"], bool(pb["fused"])))
    assert got == S.BLOCKING_CLASSES, got ^ S.BLOCKING_CLASSES


@pytest.fixture(scope="module")
def clips(oracle):
    pcm = oracle.synth(78, 0, 64)
    pcm.setflags(write=False)
    return pcm


@pytest.mark.parametrize("twin", (False, True), ids=("int8", "f32"))
@pytest.mark.parametrize("name", S.E2E_SPECS)
def test_batch_call_from_pcm(name, twin, gpu_models, oracle, clips, fixture_npz):
    """kws_run_classifier_batch_device on 64 synth clips: features, the int8 input tensor and scores against OracleModel.run_batch"""
    import torch
    gm = gpu_models(name, twin)
    es, ef, eq = D.oracle_model(oracle, S.strided_twin(name) if twin else S.strided_blob(name)).run_batch(clips, want_features=True)
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
        assert np.abs(s - es).max() <= F32_SCORE_TOL
    else:
        assert np.array_equal(d_q.cpu().numpy(), eq)
        assert np.array_equal(bits(s), bits(es))
    # ... and the fixture's rows (the reference's): the first N_SYNTH inputs of strided_features() are feature matrices of synth clips
    x = S.strided_features(name)
    if twin:
        s2, _ = run_f32(gm, x)
        assert np.abs(s2 - fixture_npz[name + "/fscores"]).max() <= F32_SCORE_TOL
    else:
        om = D.oracle_model(oracle, S.strided_blob(name))
        q = np.stack([om.quantize_input(r) for r in x])
        assert np.array_equal(gm.nn_batch(q)[3], fixture_npz[name + "/scores"])


@pytest.mark.parametrize("twin", (False, True), ids=("int8", "f32"))
@pytest.mark.parametrize("name", S.WAVE_SPECS)
def test_second_and_later_clips_per_wave(name, twin, pkg, gpu_models, expected):
    """A batch of 2 x resident + 37 inputs (resident: what the grid holds before a wave loops -- int8: one workgroup of at most 16 waves per CU; float:
    CUs x workgroups per CU x waves), so every wave serves a second and a third clip: padding rows of the previous clip or block left behind by a strided
    walk would show here.  The rows repeat the 64 reference inputs in a shuffled order; EVERY clip is compared with the oracle's output for its row."""
    import torch
    gm = gpu_models(name, twin)
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    if twin:
        pb = plan_blocking(pkg, gm, 0)
        resident = n_cu * max(1, (160 * 1024) // pb["smem"]) * pb["waves"]
    else:
        resident = n_cu * 16
    assert resident <= 16 * 1024 + 4096, (name, resident)
    B = 2 * resident + 37
    idx = np.random.default_rng(479).integers(0, S.N_INPUTS, B)
    _, _, _, last, _, _ = D.graph_layout(S.strided_blob(name))
    if twin:
        ftaps, fscores = expected(name, True)
        s, lg = run_f32(gm, S.strided_features(name)[idx])
        wrong = np.nonzero((bits(lg) != bits(ftaps[last][idx])).any(axis=1) | (np.abs(s - fscores[idx]) > F32_SCORE_TOL).any(axis=1))[0]
    else:
        q, taps, out_q, scores = expected(name)
        s, tp, tf, to = gm.nn_batch(q[idx])
        want = np.concatenate([taps[i] for i in D.block_outputs(S.strided_blob(name))], axis=1)
        wrong = np.nonzero((tp != want[idx]).any(axis=1) | (to != out_q[idx]).any(axis=1) | (bits(s) != bits(scores[idx])).any(axis=1))[0]
    assert wrong.size == 0, (name, B, resident, wrong.size, wrong[:8].tolist())


def test_sdk_run_classifier_and_run_inference(pkg, gpu_models, oracle, clips):
    """s2_k3 as the default model behind the SDK's run_classifier (from a signal) and run_inference (from a feature matrix), against the oracle"""
    gm = gpu_models("s2_k3")
    om = D.oracle_model(oracle, S.strided_blob("s2_k3"))
    es, ef, _ = om.run_batch(clips[5:6], want_features=True)
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
        assert np.array_equal(bits(got), bits(es[0]))
        fm = np.ascontiguousarray(ef[0], np.float32)
        mat = pkg.Matrix(buffer=fm.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), rows=1, cols=fm.size)
        res2 = pkg.result_struct(gm.n_labels)()
        assert pkg.lib().run_inference(ctypes.byref(mat), ctypes.byref(res2), False) == 0
        got2 = np.float32([res2.classification[i].value for i in range(gm.n_labels)])
        assert np.array_equal(bits(got2), bits(es[0]))
    finally:
        gpu_models("l476_no_yes.kwsm").set_default()


def test_bank_with_a_stride_1_member(pkg, gpu_models, clips):
    """{s2_k3, the shipped l476_no_yes (matrix-core kernel), the float twin of s2_k3} behind one front end: each member's scores equal its own call's"""
    import torch
    members = [gpu_models("s2_k3"), gpu_models("l476_no_yes.kwsm"), gpu_models("s2_k3", True)]
    B = clips.shape[0]
    d_pcm = torch.from_numpy(np.ascontiguousarray(clips)).cuda()
    own = []
    for gm in members:
        d_s = torch.empty((B, gm.n_labels), dtype=torch.float32, device="cuda")
        gm.run_classifier_batch_device(d_pcm.data_ptr(), B, d_s.data_ptr())
        torch.cuda.synchronize()
        own.append(d_s.cpu().numpy())
    bank = pkg.Bank(members)
    try:
        outs = [torch.empty((B, gm.n_labels), dtype=torch.float32, device="cuda") for gm in members]
        bank.run_classifier_batch_device(d_pcm.data_ptr(), B, [t.data_ptr() for t in outs])
        torch.cuda.synchronize()
        for k, t in enumerate(outs):
            assert np.array_equal(bits(t.cpu().numpy()), bits(own[k])), k
    finally:
        bank.close()


def test_ragged_call(gpu_models, oracle, clips):
    """kws_run_classifier_ragged_device on s2_k3: three clips of their own lengths, each against the oracle on that clip"""
    import torch
    gm = gpu_models("s2_k3")
    om = D.oracle_model(oracle, S.strided_blob("s2_k3"))
    lengths = np.array([16000, 12000, 9920], np.uint64)
    offsets = np.array([0, 16000, 32000], np.uint64)
    pcm = np.ascontiguousarray(clips[:3].reshape(-1))
    d_pcm = torch.from_numpy(pcm).cuda()
    d_s = torch.empty((3, gm.n_labels), dtype=torch.float32, device="cuda")
    gm.run_classifier_ragged_device(d_pcm.data_ptr(), offsets, lengths, d_s.data_ptr())
    torch.cuda.synchronize()
    s = d_s.cpu().numpy()
    for i in range(3):
        e = om.run_batch(pcm[int(offsets[i]):int(offsets[i] + lengths[i])][None])
        if isinstance(e, int):
            pytest.fail("the oracle refuses a clip of %d samples (rc %d)" % (int(lengths[i]), e))
        assert np.array_equal(bits(s[i]), bits(e[0])), i


def test_slide_equals_the_batch_call(gpu_models, clips):
    """d2_k3 over one 2 s recording at hop 1600: every row equals the batch call on that window"""
    import torch
    gm = gpu_models("d2_k3")
    rec = np.ascontiguousarray(clips[:2].reshape(-1))
    hop = 1600
    n = gm.slide_window_count(rec.size, hop)
    assert n == (rec.size - 16000) // hop + 1
    d = torch.from_numpy(rec).cuda()
    d_s = torch.empty((n, gm.n_labels), dtype=torch.float32, device="cuda")
    gm.slide_recordings_device(d.data_ptr(), [0], [rec.size], hop, d_s.data_ptr())
    wins = np.stack([rec[i * hop:i * hop + 16000] for i in range(n)])
    d_w = torch.from_numpy(np.ascontiguousarray(wins)).cuda()
    d_b = torch.empty((n, gm.n_labels), dtype=torch.float32, device="cuda")
    gm.run_classifier_batch_device(d_w.data_ptr(), n, d_b.data_ptr())
    torch.cuda.synchronize()
    assert np.array_equal(bits(d_s.cpu().numpy()), bits(d_b.cpu().numpy()))


@pytest.mark.parametrize("twin", (True, False), ids=("f32", "int8"))
def test_fast_mode_is_refused(twin, pkg, oracle, clips):
    """kws_set_mode(KWS_MODE_FAST) on s2_k3: KWS_ERROR_UNSUPPORTED_MODEL with a message, and the handle goes on serving KWS_MODE_EXACT"""
    import torch
    blob = S.strided_twin("s2_k3") if twin else S.strided_blob("s2_k3")
    gm = pkg.Model(blob=blob)
    try:
        with pytest.raises(pkg.KwsError) as ei:
            gm.set_mode(pkg.MODE_FAST)
        assert ei.value.code == -18 and "strided or dilated" in str(ei.value)
        with pytest.raises(pkg.KwsError) as ei:                             # no fast plan, no gain calibrated on the wrong geometry
            gm.fast_tolerance()
        assert ei.value.code == -18
        es = D.oracle_model(oracle, blob).run_batch(clips[:16])
        d_pcm = torch.from_numpy(np.ascontiguousarray(clips[:16])).cuda()
        d_s = torch.empty((16, gm.n_labels), dtype=torch.float32, device="cuda")
        gm.run_classifier_batch_device(d_pcm.data_ptr(), 16, d_s.data_ptr())
        torch.cuda.synchronize()
        s = d_s.cpu().numpy()
        assert np.abs(s - es).max() <= F32_SCORE_TOL if twin else np.array_equal(bits(s), bits(es))
    finally:
        gm.close()


def test_refusal_messages(pkg):
    """what DESIGN 4.15 leaves out: -18 from kws_create, the message naming the node and the reason (int8 and float)"""
    import dequantize_model
    from test_strided_graphs_host import REFUSED
    says = {"stride_h_2": "stride_h", "dil_h_2": "dilation_height_factor", "dw_same_dilated": "depthwise_conv.cc:489-492", "out_rows": "output shape",
            "stride_0": "1 <= stride <= input width", "stride_neg": "1 <= stride", "stride_past_rows": "1 <= stride <= input width",
            "stride_2_30": "1 <= stride", "dil_0": "dilation", "dil_neg": "dilation", "dil_int_max": "dilation", "dil_4096": "dilation", "lds": "LDS"}
    for key, spec in REFUSED.items():
        blob = synth_model_blob(**spec)
        for b in (blob, dequantize_model.dequantize(blob)):
            with pytest.raises(pkg.KwsError) as ei:
                pkg.Model(blob=b)
            assert ei.value.code == -18 and says[key] in str(ei.value), (key, str(ei.value))
            if key != "lds":
                assert "conv 1" in str(ei.value) or "conv 0" in str(ei.value) or "conv " in str(ei.value), str(ei.value)


# ---- routing of what was served before -------------------------------------------------------------------------------------------------------------
# kws_nn_kernel_name of the shipped models and of every SYNTH_SPECS / DENSE_SPECS graph (int8; "_f32": its float twin), recorded from the parent commit
PARENT_KERNELS = {
    "d_c1_h48_h16": "kws_dense_i8_kernel",
    "d_c1_h48_h16_f32": "kws_dense_f32_kernel",
    "d_c1w_h32": "kws_dense_i8_kernel",
    "d_c1w_h32_f32": "kws_dense_f32_kernel",
    "d_c2_h64": "kws_dense_i8_kernel",
    "d_c2_h64_f32": "kws_dense_f32_kernel",
    "d_d0_h20_h10": "kws_dense_i8_kernel",
    "d_d0_h20_h10_f32": "kws_dense_f32_kernel",
    "d_d0_l48": "kws_dense_i8_kernel",
    "d_d0_l48_f32": "kws_dense_f32_kernel",
    "d_d0_logreg": "kws_dense_i8_kernel",
    "d_d0_logreg_f32": "kws_dense_f32_kernel",
    "d_d0_m40_h128": "kws_dense_i8_kernel",
    "d_d0_m40_h128_f32": "kws_dense_f32_kernel",
    "d_d0_mfe_h32": "kws_dense_i8_kernel",
    "d_d0_mfe_h32_f32": "kws_dense_f32_kernel",
    "d_d0_q_inzp_127": "kws_dense_i8_kernel",
    "d_d0_q_inzp_127_f32": "kws_dense_f32_kernel",
    "d_d0_q_inzp_m128": "kws_dense_i8_kernel",
    "d_d0_q_inzp_m128_f32": "kws_dense_f32_kernel",
    "d_d0_q_mult_1_37": "kws_dense_i8_kernel",
    "d_d0_q_mult_1_37_f32": "kws_dense_f32_kernel",
    "d_d0_q_mult_one": "kws_dense_i8_kernel",
    "d_d0_q_mult_one_f32": "kws_dense_f32_kernel",
    "d_d0_q_no_bias": "kws_dense_i8_kernel",
    "d_d0_q_no_bias_f32": "kws_dense_f32_kernel",
    "d_d0_q_relu_n1": "kws_dense_i8_kernel",
    "d_d0_q_relu_n1_f32": "kws_dense_f32_kernel",
    "d_d0_q_wzp_m5": "kws_dense_i8_kernel",
    "d_d0_q_wzp_m5_f32": "kws_dense_f32_kernel",
    "d_d0_q_wzp_p5": "kws_dense_i8_kernel",
    "d_d0_q_wzp_p5_f32": "kws_dense_f32_kernel",
    "d_d0_u1": "kws_dense_i8_kernel",
    "d_d0_u15": "kws_dense_i8_kernel",
    "d_d0_u15_f32": "kws_dense_f32_kernel",
    "d_d0_u16": "kws_dense_i8_kernel",
    "d_d0_u16_f32": "kws_dense_f32_kernel",
    "d_d0_u17": "kws_dense_i8_kernel",
    "d_d0_u17_f32": "kws_dense_f32_kernel",
    "d_d0_u1_f32": "kws_dense_f32_kernel",
    "d_d0_u255": "kws_dense_i8_kernel",
    "d_d0_u255_f32": "kws_dense_f32_kernel",
    "d_d0_u256": "kws_dense_i8_kernel",
    "d_d0_u256_f32": "kws_dense_f32_kernel",
    "d_d0_u63": "kws_dense_i8_kernel",
    "d_d0_u63_f32": "kws_dense_f32_kernel",
    "d_d0_u64": "kws_dense_i8_kernel",
    "d_d0_u64_f32": "kws_dense_f32_kernel",
    "d_d0_u65": "kws_dense_i8_kernel",
    "d_d0_u65_f32": "kws_dense_f32_kernel",
    "m_cfg2_mfcc40_f32": "kws_nn_f32_kernel",
    "m_cfg2_mfcc40_int8": "kws_nn_mfma_kernel",
    "m_cfg5_dscnn_mfcc40_f32": "kws_nn_f32_kernel",
    "m_cfg5_dscnn_mfcc40_int8": "kws_nn_kernel",
    "m_l432_trick_or_treat": "kws_nn_mfma_kernel",
    "m_l476_no_yes": "kws_nn_mfma_kernel",
    "m_l476_no_yes_f32": "kws_nn_f32_kernel",
    "s_cfg5_dscnn": "kws_nn_kernel",
    "s_cfg5_dscnn_f32": "kws_nn_f32_kernel",
    "s_dscnn_a": "kws_nn_kernel",
    "s_dscnn_a_f32": "kws_nn_f32_kernel",
    "s_dscnn_b": "kws_nn_kernel",
    "s_dscnn_b_f32": "kws_nn_f32_kernel",
    "s_ei_default": "kws_nn_kernel",
    "s_ei_default40": "kws_nn_kernel",
    "s_ei_default40_f32": "kws_nn_f32_kernel",
    "s_ei_default_f32": "kws_nn_f32_kernel",
    "s_ei_default_same": "kws_nn_kernel",
    "s_ei_default_same_f32": "kws_nn_f32_kernel",
    "s_f40c40": "kws_nn_kernel",
    "s_f40c40_f32": "kws_nn_f32_kernel",
    "s_mfma_mix": "kws_nn_kernel",
    "s_mfma_mix2": "kws_nn_kernel",
    "s_mfma_mix2_f32": "kws_nn_f32_kernel",
    "s_mfma_mix_f32": "kws_nn_f32_kernel",
    "s_seed1": "kws_nn_mfma_kernel",
    "s_seed1_f32": "kws_nn_f32_kernel",
    "s_seed2": "kws_nn_kernel",
    "s_seed2_f32": "kws_nn_f32_kernel",
    "s_seed4": "kws_nn_mfma_kernel",
    "s_seed4_f32": "kws_nn_f32_kernel",
    "s_seed5": "kws_nn_mfma_kernel",
    "s_seed5_f32": "kws_nn_f32_kernel",
    "s_seed6": "kws_nn_kernel",
    "s_seed6_f32": "kws_nn_f32_kernel",
    "s_seed7": "kws_nn_kernel",
    "s_seed7_f32": "kws_nn_f32_kernel",
}


def test_routes_of_the_graphs_served_before(pkg):
    import dequantize_model
    got = {}
    for fn in sorted(os.listdir(MODELS)):
        if fn.endswith(".kwsm"):
            gm = pkg.Model(os.path.join(MODELS, fn))
            got["m_" + fn[:-5]] = gm.nn_kernel
            gm.close()
    blobs = {"s_" + k: synth_model_blob(**v) for k, v in SYNTH_SPECS.items()}
    blobs.update({"d_" + k: D.dense_blob(k) for k in D.DENSE_SPECS})
    for k, blob in blobs.items():
        for suffix, b in (("", blob), ("_f32", dequantize_model.dequantize(blob))):
            gm = pkg.Model(blob=b)
            got[k + suffix] = gm.nn_kernel
            gm.close()
    assert got == PARENT_KERNELS, {k: (got.get(k), PARENT_KERNELS.get(k)) for k in set(got) | set(PARENT_KERNELS) if got.get(k) != PARENT_KERNELS.get(k)}
