"""-m gpu: residual graphs through the C ABI, against the oracle (pinned to the reference by tests/golden/residual_graphs.npz,
tests/test_residual_graphs_host.py): the residual trunk + dense kernels alone (every step output, bit for bit), all 65 536 int8 operand pairs of the ADD,
batches in which every wave serves several clips, a clip list and a chunked hand-off, the entry points from PCM (batch, SDK, bank, ragged, slide, scan),
the fast-mode refusal, the refusals' messages, and the kernels of the graphs served before."""
import ctypes
import os
import sys

import numpy as np
import pytest

import dense_testlib as D
import residual_testlib as T
from kws_testlib import MODELS, ROOT, bits

pytestmark = pytest.mark.gpu

F32_SCORE_TOL = 1e-6           # the project's bar for exact-mode float32 scores (the float softmax uses the device expf)
NAMES = list(T.RES_SPECS)
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
                made[key] = pkg.Model(blob=T.res_twin(name) if twin else T.res_blob(name))
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
            made[key] = (T.oracle_f32(oracle, T.res_twin(name), T.res_twin_features()) if twin else T.oracle_int8(oracle, T.res_blob(name), T.res_features()))
        return made[key]

    return get


@pytest.fixture(scope="module")
def fixture_npz():
    return np.load(T.GOLDEN_RESIDUAL)


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


def check_int8_taps(name, gm, q, taps, out_q, scores):
    """kws_nn_batch_device with every tap against the oracle's tensors, tensor by tensor so that a failure names the step"""
    blob = T.res_blob(name)
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
    assert gm.residual_add_count == T.N_ADDS[name] and gm.conv2d_block_count == 0 and not gm.is_float
    _, _, hidden, _, _, _ = D.graph_layout(T.res_blob(name))
    assert gm.dense_layer_count == len(hidden) + 1
    check_int8_taps(name, gm, q, taps, out_q, scores)


@pytest.mark.parametrize("name", T.ALL_PAIRS)
def test_add_int8_all_operand_pairs(name, gpu_models, oracle, fixture_npz):
    """all_pairs_rows(): every one of the 65 536 (a, b) operand pairs through the ADD step, its output and everything behind it bit for bit"""
    q, taps, out_q, scores = T.oracle_int8(oracle, T.res_blob(name), q=T.all_pairs_rows())
    add_id = T.step_outputs(T.res_blob(name))[1]
    assert [D.digest(taps[add_id]), D.digest(out_q)] == [int(v) for v in fixture_npz[name + "/pairs"]]
    check_int8_taps(name, gpu_models(name), q, taps, out_q, scores)


@pytest.mark.parametrize("name", NAMES)
def test_network_float32(name, gpu_models, expected, fixture_npz):
    """kws_nn_f32_batch_device on the twin: logits bit for bit (NaN by position), scores within 1e-6 of the oracle"""
    gm = gpu_models(name, twin=True)
    ftaps, fscores = expected(name, twin=True)
    assert T.same_bits_nan_by_position(fscores, fixture_npz[name + "/fscores"].view(np.float32))
    assert gm.is_float and gm.nn_kernel == KERNEL_F32, gm.nn_kernel
    assert gm.residual_add_count == T.N_ADDS[name] and gm.conv2d_block_count == 0
    _, _, _, last, _, _ = D.graph_layout(T.res_blob(name))
    s, lg = run_f32(gm, T.res_twin_features())
    assert T.same_bits_nan_by_position(lg, ftaps[last]), name
    err = score_error(s, fscores)
    print(name, "max |score - oracle| = %.3g" % err)
    assert err <= F32_SCORE_TOL, name


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
    blob = T.res_blob(name)
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


@pytest.mark.parametrize("twin", (False, True), ids=("int8", "f32"))
def test_clip_list_and_chunked_handoff(twin, dev_pkg, expected):
    """tc_identity (784 hand-off values per clip) on the development build with a hand-off buffer of 16 clips: the 40 reference rows walk three chunks, and
    a clip list of 21 entries (the route batch_network_device takes) walks two.  Clips the list does not name keep their sentinel scores"""
    import torch
    name = "tc_identity"
    per_clip = 49 * 16 * (4 if twin else 1)
    old = os.environ.get("KWS_DEV_HANDOFF_BYTES")
    os.environ["KWS_DEV_HANDOFF_BYTES"] = str(16 * per_clip)
    try:
        gm = dev_pkg.Model(blob=T.res_twin(name) if twin else T.res_blob(name))
    finally:
        if old is None:
            os.environ.pop("KWS_DEV_HANDOFF_BYTES", None)
        else:
            os.environ["KWS_DEV_HANDOFF_BYTES"] = old
    try:
        if twin:
            _, want = expected(name, True)
            want = want[:T.N_STD]
            d_in = torch.from_numpy(np.ascontiguousarray(T.res_features())).cuda()
            d_s = torch.empty((T.N_STD, gm.n_labels), dtype=torch.float32, device="cuda")
            gm.nn_f32_batch_device(d_in.data_ptr(), T.N_STD, d_s.data_ptr())
        else:
            q, _, _, want = expected(name)
            d_in = torch.from_numpy(np.ascontiguousarray(q)).cuda()
            d_s = torch.empty((T.N_STD, gm.n_labels), dtype=torch.float32, device="cuda")
            gm.nn_batch_device(d_in.data_ptr(), T.N_STD, d_s.data_ptr())
        torch.cuda.synchronize()
        s = d_s.cpu().numpy()
        assert np.abs(s - want).max() <= F32_SCORE_TOL if twin else np.array_equal(bits(s), bits(want))
        # the clip list: 21 clips in a shuffled order
        picked = np.random.default_rng(7).permutation(T.N_STD)[:21].astype(np.int32)
        d_sel = torch.from_numpy(np.concatenate([np.int32([picked.size]), picked])).cuda()
        d_s2 = torch.full((T.N_STD, gm.n_labels), -7.0, dtype=torch.float32, device="cuda")
        L = dev_pkg.lib()
        L.kws_dev_network_sel.restype = ctypes.c_int
        L.kws_dev_network_sel.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
        assert L.kws_dev_network_sel(gm.h, d_in.data_ptr(), T.N_STD, d_s2.data_ptr(), d_sel.data_ptr(), None) == 0
        torch.cuda.synchronize()
        s2 = d_s2.cpu().numpy()
        rest = np.setdiff1d(np.arange(T.N_STD), picked)
        assert np.all(s2[rest] == -7.0)
        assert np.array_equal(bits(s2[picked]), bits(s[picked]))
    finally:
        gm.close()


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
    om = D.oracle_model(oracle, T.res_twin(name) if twin else T.res_blob(name))
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


def test_bank_with_a_1d_member(pkg, gpu_models, clips):
    """{tc_res8, the shipped l476_no_yes (same DSP block, matrix-core kernel), the float twin of res2d_identity} behind one front end: each member equals
    its own call"""
    import torch
    members = [gpu_models("tc_res8"), gpu_models("l476_no_yes.kwsm"), gpu_models("res2d_identity", True)]
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
    """kws_run_classifier_ragged_device on tc_res8: three clips of their own lengths, each against the oracle on that clip"""
    import torch
    gm = gpu_models("tc_res8")
    om = D.oracle_model(oracle, T.res_blob("tc_res8"))
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


@pytest.mark.parametrize("name", T.E2E_SPECS)
def test_slide_equals_the_batch_call(name, gpu_models, clips):
    """one 2 s recording at hop 1600: every row equals the batch call on that window"""
    import torch
    gm = gpu_models(name)
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


def test_continuous_scan(gpu_models, oracle):
    """one kws_scan_recordings_device call on tc_res8 over a short recording, against the oracle's continuous mode"""
    import torch
    from scan_testlib import oracle_scan, pack, speech
    gm = gpu_models("tc_res8")
    om = D.oracle_model(oracle, T.res_blob("tc_res8"))
    recs = [speech(oracle, 93, 28000)]
    pcm, offs, lens = pack(recs, seed=4)
    W = [gm.scan_window_count(int(n)) for n in lens]
    d = torch.from_numpy(pcm).cuda()
    d_s = torch.empty((sum(W), gm.n_labels), dtype=torch.float32, device="cuda")
    gm.scan_recordings_device(d.data_ptr(), offs, lens, d_s.data_ptr())
    torch.cuda.synchronize()
    want = oracle_scan(om, recs[0])
    assert want.shape[0] == W[0] and W[0] > 0
    assert np.array_equal(bits(d_s.cpu().numpy()), bits(want))


@pytest.mark.parametrize("twin", (True, False), ids=("f32", "int8"))
def test_fast_mode_is_refused(twin, pkg, oracle, clips):
    """kws_set_mode(KWS_MODE_FAST) on tc_proj_s2: KWS_ERROR_UNSUPPORTED_MODEL with a message, and the handle goes on serving KWS_MODE_EXACT"""
    import torch
    blob = T.res_twin("tc_proj_s2") if twin else T.res_blob("tc_proj_s2")
    gm = pkg.Model(blob=blob)
    try:
        with pytest.raises(pkg.KwsError) as ei:
            gm.set_mode(pkg.MODE_FAST)
        assert ei.value.code == -18 and "residual" in str(ei.value)
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
    """what DESIGN 4.17 leaves out: -18 from kws_create, the message naming the node and the reason"""
    blobs = T.refused_blobs()
    for key, (_, which, says) in T.REFUSED.items():
        for k in [key] + [key + "_f32"] * (which == "both"):
            with pytest.raises(pkg.KwsError) as ei:
                pkg.Model(blob=blobs[k])
            msg = str(ei.value)
            assert ei.value.code == -18 and says in msg, (k, msg)
            assert any(w in msg for w in ("conv ", "pool ", "ADD ", "node ", "residual graph", "residual model")), (k, msg)


def test_graphs_served_before_keep_their_kernels(pkg):
    """kws_residual_add_count is 0 and kws_nn_kernel_name unchanged for the shipped models and one graph of each family served before"""
    from test_gpu_strided_graphs import PARENT_KERNELS
    import conv2d_testlib as C2
    import dequantize_model
    import strided_testlib as S
    from kws_testlib import SYNTH_SPECS, synth_model_blob
    got = {}
    for fn in sorted(os.listdir(MODELS)):
        if fn.endswith(".kwsm"):
            gm = pkg.Model(os.path.join(MODELS, fn))
            got["m_" + fn[:-5]] = (gm.nn_kernel, gm.residual_add_count)
            gm.close()
    blobs = {"s_dscnn_a": synth_model_blob(**SYNTH_SPECS["dscnn_a"]), "s_seed1": synth_model_blob(**SYNTH_SPECS["seed1"]),
             "d_c2_h64": D.dense_blob("c2_h64"), "d_d0_h20_h10": D.dense_blob("d0_h20_h10")}
    for k, blob in blobs.items():
        for suffix, b in (("", blob), ("_f32", dequantize_model.dequantize(blob))):
            gm = pkg.Model(blob=b)
            got[k + suffix] = (gm.nn_kernel, gm.residual_add_count)
            gm.close()
    assert got == {k: (PARENT_KERNELS[k], 0) for k in got}, got
    for blob, want in ((S.strided_blob("s2_k3"), "kws_nn_sd_kernel"), (S.strided_twin("s2_k3"), "kws_nn_f32_sd_kernel"),
                       (C2.conv2d_blob("ei_2d"), "kws_nn2d_trunk_kernel + kws_dense_i8_kernel"),
                       (C2.conv2d_twin("ei_2d"), "kws_nn2d_f32_trunk_kernel + kws_dense_f32_kernel")):
        gm = pkg.Model(blob=blob)
        assert (gm.nn_kernel, gm.residual_add_count) == (want, 0)
        gm.close()
