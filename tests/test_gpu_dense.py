"""Graphs with dense stacks on the GPU, through the C ABI, against the oracle (pinned to the reference by tests/golden/dense_l476.npz,
tests/test_dense_graphs_host.py): kws_dense_i8_kernel / kws_dense_f32_kernel alone at batch sizes around the clip tiles, the trunk hand-off, the batch
and stage calls, a bank, fast mode, and the routes of the models served before."""
import os
import sys

import numpy as np
import pytest

import dense_testlib as D
from kws_testlib import MODELS, ROOT, OracleModel, bits, special_clips

pytestmark = pytest.mark.gpu

F32_SCORE_TOL = 1e-6           # the project's bar for exact-mode float32 scores (the float softmax uses the device expf)
BATCHES = (1, 15, 16, 17, 63, 64, 65, 1000, 4099)      # clip-tile tails (16 per wave, 64 per workgroup) and more than one tile per workgroup
NAMES = list(D.DENSE_SPECS)
CALL_MODELS = ("d0_h20_h10", "c2_h64", "d0_m40_h128", "d0_mfe_h32")


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
                made[key] = pkg.Model(blob=D.dense_twin(name) if twin else D.dense_blob(name))
        return made[key]

    yield get
    for m in made.values():
        m.close()


@pytest.fixture(scope="module")
def expected(oracle):
    """per model: the oracle's tensors on dense_features(), computed once"""
    made = {}

    def get(name, twin=False):
        key = (name, twin)
        if key not in made:
            f = D.dense_features(name)
            made[key] = D.oracle_f32(oracle, D.dense_twin(name), f) if twin else D.oracle_int8(oracle, D.dense_blob(name), f)
        return made[key]

    return get


@pytest.fixture(scope="module")
def fixture_npz():
    return np.load(D.GOLDEN_DENSE)


def _rows(B):
    """which of the N_INPUTS reference rows clip i of a batch of B is (every row appears, in an order that differs from tile to tile)"""
    return (np.arange(B) * 37 + (np.arange(B) // 64) * 5) % D.N_INPUTS


@pytest.mark.parametrize("name", NAMES)
def test_network_int8_all_taps(name, gpu_models, expected, fixture_npz):
    """kws_nn_batch_device with every tap: hidden tensors (behind the pooled outputs of tap_pooled), tap_fc, tap_out and scores, bit for bit, every clip"""
    gm = gpu_models(name)
    q, taps, out_q, scores = expected(name)
    assert np.array_equal(out_q, fixture_npz[name + "/scores"])              # the oracle is the reference's here too
    _, _, hidden, last, _, _ = D.graph_layout(D.dense_blob(name))
    assert gm.dense_layer_count == len(hidden) + 1 and gm.nn_kernel == "kws_dense_i8_kernel"
    hid = np.concatenate([taps[i] for i in hidden], axis=1) if hidden else np.zeros((D.N_INPUTS, 0), np.int8)
    blk = D.block_outputs(D.dense_blob(name))               # the conv blocks' share of the tap: written by the trunk form of kws_nn_kernel
    trunk = np.concatenate([taps[i] for i in blk], axis=1) if blk else np.zeros((D.N_INPUTS, 0), np.int8)
    assert gm.pooled_tap_bytes == trunk.shape[1] + hid.shape[1]
    for B in BATCHES + D.EXTRA_BATCHES.get(name, ()):
        r = _rows(B)
        s, tp, tf, to = gm.nn_batch(q[r])
        assert np.array_equal(tp[:, :trunk.shape[1]], trunk[r]), (name, B)
        assert np.array_equal(tp[:, trunk.shape[1]:], hid[r]), (name, B)
        assert np.array_equal(tf, taps[last][r]), (name, B)
        assert np.array_equal(to, out_q[r]), (name, B)
        assert np.array_equal(bits(s), bits(scores[r])), (name, B)


@pytest.mark.parametrize("name", NAMES)
def test_network_float32(name, gpu_models, expected, fixture_npz):
    """kws_nn_f32_batch_device on the twin: logits bit for bit, scores within 1e-6"""
    import torch
    gm = gpu_models(name, twin=True)
    ftaps, fscores = expected(name, twin=True)
    assert np.array_equal(bits(fscores), bits(fixture_npz[name + "/fscores"]))
    _, _, hidden, last, _, _ = D.graph_layout(D.dense_blob(name))
    assert gm.is_float and gm.dense_layer_count == len(hidden) + 1 and gm.nn_kernel == "kws_dense_f32_kernel"
    f = D.dense_features(name)
    for B in BATCHES + D.EXTRA_BATCHES.get(name, ()):
        r = _rows(B)
        d_f = torch.from_numpy(f[r]).cuda()
        d_s = torch.full((B + 1, gm.n_labels), -7.0, dtype=torch.float32, device="cuda")
        d_l = torch.full((B + 1, gm.n_labels), -7.0, dtype=torch.float32, device="cuda")
        gm.nn_f32_batch_device(d_f.data_ptr(), B, d_s.data_ptr(), d_l.data_ptr())
        torch.cuda.synchronize()
        s, lg = d_s.cpu().numpy(), d_l.cpu().numpy()
        assert np.all(s[B] == -7.0) and np.all(lg[B] == -7.0)                 # nothing behind the batch is written
        assert np.array_equal(bits(lg[:B]), bits(ftaps[last][r])), (name, B)
        print(name, B, "max |score - oracle| = %.3g" % float(np.abs(s[:B] - fscores[r]).max()))
        assert np.abs(s[:B] - fscores[r]).max() <= F32_SCORE_TOL, (name, B)


@pytest.fixture(scope="module")
def clips(oracle):
    pcm = np.concatenate([oracle.synth(77, 0, 256), np.stack(list(special_clips().values()))])
    pcm.setflags(write=False)
    return pcm


@pytest.fixture(scope="module")
def oracle_calls(oracle, clips):
    """(model, twin) -> the oracle's (scores, features, q) of the whole clips batch"""
    made = {}

    def get(name, twin=False):
        key = (name, twin)
        if key not in made:
            m = D.oracle_model(oracle, D.dense_twin(name) if twin else D.dense_blob(name))
            made[key] = m.run_batch(clips, want_features=True)
        return made[key]

    return get


def _same_or_both_nan(a, b):
    return np.array_equal(bits(a), bits(b)) or np.array_equal(np.where(np.isnan(a), np.float32(0), a), np.where(np.isnan(b), np.float32(0), b))


@pytest.mark.parametrize("twin", (False, True), ids=("int8", "f32"))
@pytest.mark.parametrize("name", CALL_MODELS)
def test_batch_call(name, twin, gpu_models, oracle_calls, clips):
    """kws_run_classifier_batch_device: features, the int8 input tensor and scores of 256 synth clips and the special clips"""
    import torch
    gm = gpu_models(name, twin)
    es, ef, eq = oracle_calls(name, twin)
    B = clips.shape[0]
    d_pcm = torch.from_numpy(np.ascontiguousarray(clips)).cuda()
    d_s = torch.empty((B, gm.n_labels), dtype=torch.float32, device="cuda")
    d_f = torch.empty((B, gm.n_features), dtype=torch.float32, device="cuda")
    d_q = torch.empty((B, gm.n_features), dtype=torch.int8, device="cuda")
    gm.run_classifier_batch_device(d_pcm.data_ptr(), B, d_s.data_ptr(), d_f.data_ptr(), None if twin else d_q.data_ptr())
    torch.cuda.synchronize()
    s, f = d_s.cpu().numpy(), d_f.cpu().numpy()
    ok = ~np.isnan(ef).any(axis=1)                          # (a constant clip through the MFE block: the reference's 0 x inf NaNs)
    assert np.array_equal(bits(f[ok]), bits(ef[ok]))
    if twin:
        assert np.abs(s[ok] - es[ok]).max() <= F32_SCORE_TOL
    else:
        assert np.array_equal(d_q.cpu().numpy()[ok], eq[ok])
        assert np.array_equal(bits(s[ok]), bits(es[ok]))


@pytest.mark.parametrize("twin", (False, True), ids=("int8", "f32"))
@pytest.mark.parametrize("name", ("c2_h64", "d0_h20_h10"))
def test_stage_call(name, twin, gpu_models, oracle_calls, clips):
    """kws_mfcc_batch_device + kws_cmvn_inference_batch_device: cmvnw + quantise, then the network in a launch of its own"""
    import torch
    gm = gpu_models(name, twin)
    es, ef, eq = oracle_calls(name, twin)
    B = clips.shape[0]
    d_pcm = torch.from_numpy(np.ascontiguousarray(clips)).cuda()
    d_m = torch.empty((B, gm.n_features), dtype=torch.float32, device="cuda")
    d_s = torch.empty((B, gm.n_labels), dtype=torch.float32, device="cuda")
    d_f = torch.empty((B, gm.n_features), dtype=torch.float32, device="cuda")
    gm.mfcc_batch_device(d_pcm.data_ptr(), B, d_m.data_ptr())
    gm.cmvn_inference_batch_device(d_m.data_ptr(), B, d_s.data_ptr(), d_f.data_ptr())
    torch.cuda.synchronize()
    assert np.array_equal(bits(d_f.cpu().numpy()), bits(ef))
    if twin:
        assert np.abs(d_s.cpu().numpy() - es).max() <= F32_SCORE_TOL
    else:
        assert np.array_equal(bits(d_s.cpu().numpy()), bits(es))


def test_sdk_run_classifier_and_scan(pkg, gpu_models, oracle, clips):
    """c2_h64 behind the SDK's run_classifier (one clip) and one kws_scan_recordings_device call over two short recordings, against the oracle"""
    import ctypes
    import torch
    from scan_testlib import oracle_scan, pack, speech
    gm = gpu_models("c2_h64")
    om = D.oracle_model(oracle, D.dense_blob("c2_h64"))
    gm.set_default()
    try:
        buf = clips[3].astype(np.float32) / np.float32(32768)

        @pkg.GET_DATA_FN
        def get_data(offset, length, out):
            ctypes.memmove(out, buf[offset:offset + length].ctypes.data, 4 * length)
            return 0
        sig = pkg.Signal(get_data=get_data, total_length=16000)
        res = pkg.result_struct(gm.n_labels)()
        assert pkg.lib().run_classifier(ctypes.byref(sig), ctypes.byref(res), False) == 0
        got = np.float32([res.classification[i].value for i in range(gm.n_labels)])
        assert np.array_equal(bits(got), bits(om.run_batch(clips[3:4])[0]))
    finally:
        gpu_models("l476_no_yes.kwsm").set_default()
    recs = [speech(oracle, 91, 24000), speech(oracle, 92, 36321)]
    pcm, offs, lens = pack(recs, seed=3)
    W = [gm.scan_window_count(int(n)) for n in lens]
    d = torch.from_numpy(pcm).cuda()
    d_s = torch.empty((sum(W), gm.n_labels), dtype=torch.float32, device="cuda")
    gm.scan_recordings_device(d.data_ptr(), offs, lens, d_s.data_ptr())
    torch.cuda.synchronize()
    s, at = d_s.cpu().numpy(), 0
    for rec, w in zip(recs, W):
        want = oracle_scan(om, rec)
        assert want.shape[0] == w and w > 0
        assert np.array_equal(bits(s[at:at + w]), bits(want))
        at += w


def test_ragged_call(gpu_models, oracle, clips):
    """kws_run_classifier_ragged_device on c2_h64: four clips of their own lengths, each against the oracle on that clip"""
    import torch
    gm = gpu_models("c2_h64")
    om = D.oracle_model(oracle, D.dense_blob("c2_h64"))
    lengths = np.array([16000, 12000, 9920, 16000], np.uint64)
    offsets = np.array([0, 16000, 32000, 48000], np.uint64)
    pcm = np.ascontiguousarray(clips[:4].reshape(-1))
    d_pcm = torch.from_numpy(pcm).cuda()
    d_s = torch.empty((4, gm.n_labels), dtype=torch.float32, device="cuda")
    gm.run_classifier_ragged_device(d_pcm.data_ptr(), offsets, lengths, d_s.data_ptr())
    torch.cuda.synchronize()
    s = d_s.cpu().numpy()
    for i in range(4):
        e = om.run_batch(pcm[int(offsets[i]):int(offsets[i] + lengths[i])][None])
        if isinstance(e, int):
            pytest.fail("the oracle refuses a clip of %d samples (rc %d)" % (int(lengths[i]), e))
        assert np.array_equal(bits(s[i]), bits(e[0])), i


def test_bank(pkg, gpu_models, clips):
    """{l476_no_yes, c2_h64, d0_h20_h10, the float twin of d0_h20_h10} behind one front end: every member bit-identical to its own call"""
    import torch
    members = [gpu_models("l476_no_yes.kwsm"), gpu_models("c2_h64"), gpu_models("d0_h20_h10"), gpu_models("d0_h20_h10", True)]
    B = 131
    d_pcm = torch.from_numpy(np.ascontiguousarray(clips[:B])).cuda()
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


def test_fast_mode_int8(pkg, oracle, clips):
    """d0_h20_h10 in KWS_MODE_FAST: the plain fast front end + the dense launch; the network is exact from the int8 tensor the call returns"""
    import torch
    gm = pkg.Model(blob=D.dense_blob("d0_h20_h10"))
    try:
        gm.set_mode(pkg.MODE_FAST)
        assert not gm.fast_is_fused
        om = D.oracle_model(oracle, D.dense_blob("d0_h20_h10"))
        B = clips.shape[0]
        d_pcm = torch.from_numpy(np.ascontiguousarray(clips)).cuda()
        d_s = torch.empty((B, gm.n_labels), dtype=torch.float32, device="cuda")
        d_f = torch.empty((B, gm.n_features), dtype=torch.float32, device="cuda")
        d_q = torch.empty((B, gm.n_features), dtype=torch.int8, device="cuda")
        gm.run_classifier_batch_device(d_pcm.data_ptr(), B, d_s.data_ptr(), d_f.data_ptr(), d_q.data_ptr())
        torch.cuda.synchronize()
        q, s = d_q.cpu().numpy(), d_s.cpu().numpy()
        e = np.stack([om.dequantize(om.nn_invoke(row)) for row in q])
        assert np.array_equal(bits(s), bits(e))
    finally:
        gm.close()


def test_fast_mode_float32_is_refused(pkg):
    gm = pkg.Model(blob=D.dense_twin("d0_h20_h10"))
    try:
        with pytest.raises(pkg.KwsError) as ei:
            gm.set_mode(pkg.MODE_FAST)
        assert ei.value.code == -18 and "dense" in str(ei.value)
        assert gm.fast_tolerance()["calibrated"] == 0
    finally:
        gm.close()


def test_selection_list_across_handoff_chunks(dev_pkg, oracle, clips):
    """c2_h64 in KWS_MODE_FAST on the development build with a hand-off buffer of 160 bytes (16 clips of its 10 values): the clips the fast kernel hands
    back (digital silence and DC among them, more than two chunks' worth) re-run through the selection list, chunk after chunk of list entries, in
    the trunk and the dense kernel.  Scores equal the oracle's network on the int8 tensor the call returns, bit for bit, for every clip"""
    import torch
    old = os.environ.get("KWS_DEV_HANDOFF_BYTES")
    os.environ["KWS_DEV_HANDOFF_BYTES"] = "160"
    try:
        gm = dev_pkg.Model(blob=D.dense_blob("c2_h64"))
    finally:
        if old is None:
            os.environ.pop("KWS_DEV_HANDOFF_BYTES", None)
        else:
            os.environ["KWS_DEV_HANDOFF_BYTES"] = old
    try:
        om = D.oracle_model(oracle, D.dense_blob("c2_h64"))
        # clips a fast tier is unlikely to keep: silence, DC levels, one-LSB noise, clips that go silent half way
        rng = np.random.default_rng(9)
        hard = np.zeros((64, clips.shape[1]), np.int16)
        hard[16:32] = (np.arange(16, dtype=np.int16) * 1000 - 8000)[:, None]
        hard[32:48] = rng.integers(-1, 2, (16, clips.shape[1]))
        hard[48:] = clips[200:216]
        hard[48:, 8000:] = 0
        pcm = np.ascontiguousarray(np.concatenate([clips[:100], hard, clips[100:]]))
        B = pcm.shape[0]
        d_pcm = torch.from_numpy(pcm).cuda()
        outs = {}
        for mode in (dev_pkg.MODE_EXACT, dev_pkg.MODE_FAST):            # exact mode: B / 16 chunks of plain clips
            gm.set_mode(mode)
            d_s = torch.empty((B, gm.n_labels), dtype=torch.float32, device="cuda")
            d_f = torch.empty((B, gm.n_features), dtype=torch.float32, device="cuda")
            d_q = torch.empty((B, gm.n_features), dtype=torch.int8, device="cuda")
            gm.run_classifier_batch_device(d_pcm.data_ptr(), B, d_s.data_ptr(), d_f.data_ptr(), d_q.data_ptr())
            torch.cuda.synchronize()
            q, s = d_q.cpu().numpy(), d_s.cpu().numpy()
            e = np.stack([om.dequantize(om.nn_invoke(row)) for row in q])
            assert np.array_equal(bits(s), bits(e)), mode
            outs[mode] = s
        n_back = gm.fast_fallback_count()
        print("clips handed back by the fast kernel:", n_back, "of", B)
        assert n_back > 32                                               # the list is longer than two chunks
    finally:
        gm.close()


@pytest.mark.parametrize("fn", ("l476_no_yes.kwsm", "cfg2_mfcc40_f32.kwsm"))
def test_existing_routes_unchanged(fn, pkg, oracle):
    """the models served before keep their kernels: one FULLY_CONNECTED, the fused fast form, and a batch call that equals the library's own
    stage calls (the existing suite holds those to the oracle).  Exact mode: bit for bit.  Fast mode, float32: within the library's own
    score_tol of the exact stage scores.  Fast mode, int8: every score is a multiple of 1 / 256 and the network is exact from the int8 tensor on, so
    a clip's scores differ from the exact stage call's only where a feature on a rounding boundary moved one int8 step -- at most 2 of these 64
    clips, the bar (and the clips) __graft_entry__.smoke() holds the same model to"""
    import torch
    clips = oracle.synth(123, 0, 64)
    gm = pkg.Model(os.path.join(MODELS, fn))
    try:
        assert gm.dense_layer_count == 1 and gm.nn_kernel in ("kws_nn_mfma_kernel", "kws_nn_f32_kernel")
        B = 64
        d_pcm = torch.from_numpy(np.ascontiguousarray(clips[:B])).cuda()
        d_m = torch.empty((B, gm.n_features), dtype=torch.float32, device="cuda")
        d_s0 = torch.empty((B, gm.n_labels), dtype=torch.float32, device="cuda")
        d_s1 = torch.empty((B, gm.n_labels), dtype=torch.float32, device="cuda")
        gm.mfcc_batch_device(d_pcm.data_ptr(), B, d_m.data_ptr())
        gm.cmvn_inference_batch_device(d_m.data_ptr(), B, d_s0.data_ptr())
        gm.run_classifier_batch_device(d_pcm.data_ptr(), B, d_s1.data_ptr())
        torch.cuda.synchronize()
        s0 = d_s0.cpu().numpy()
        assert np.array_equal(bits(s0), bits(d_s1.cpu().numpy()))
        gm.set_mode(pkg.MODE_FAST)
        assert gm.fast_is_fused
        d_s2 = torch.empty((B, gm.n_labels), dtype=torch.float32, device="cuda")
        gm.run_classifier_batch_device(d_pcm.data_ptr(), B, d_s2.data_ptr())
        torch.cuda.synchronize()
        s2 = d_s2.cpu().numpy()
        diff = np.abs(s2 - s0)
        print(fn, "fast batch call vs exact stage calls: max |d| = %.3g, clips that differ: %d of %d" % (diff.max(), int((diff.max(axis=1) > 0).sum()), B))
        if gm.is_float:
            assert diff.max() <= gm.fast_tolerance()["score_tol"]
        else:
            assert np.array_equal(s2 * 256, np.round(s2 * 256)) and int((diff.max(axis=1) > 0).sum()) <= 2
    finally:
        gm.close()
