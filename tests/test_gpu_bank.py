"""kws_bank_*: K models with an identical DSP block scored in one call, the front end computed once.  Every member's scores against that
member's own device call in KWS_MODE_EXACT (bit for bit, float32 graphs included) and against the oracle (int8 bit-exact, float32 within
1e-6), the shared feature matrix in bits, for every kernel class a bank dispatches to: the bank's matrix-core kernel at both row widths,
the quantise pass + the generic int8 kernel, the float kernel; tuned, general-shape and MFE front ends; clips, cepstra and the slide."""
import os
import sys

import numpy as np
import pytest

from kws_testlib import MODELS, ROOT, OracleModel, bits, special_clips, synth_model_blob
from slide_testlib import MFE_KW, SENTINEL, speech

pytestmark = pytest.mark.gpu

F32_SCORE_TOL = 1e-6           # the project's bar for exact-mode float32 scores (the float softmax uses the device expf, kws.h)
AUTO, DIRECT, SHARED = 0, 1, 2
CLIP = 16000
MFCC40 = ["cfg2_mfcc40_int8.kwsm", "cfg2_mfcc40_f32.kwsm", "cfg5_dscnn_mfcc40_int8.kwsm", "cfg5_dscnn_mfcc40_f32.kwsm"]
# a generic-kernel int8 graph behind l476's DSP block (synth_model_blob's default DSP arguments are l476's)
SYNTH13 = dict(seed=7, blocks=((12, 5, 2), (6, 3, 2)), n_labels=3)
BANKS = {
    "49x13": (["l476_no_yes.kwsm", "l476_no_yes_f32.kwsm", "synth13"], 259),
    "49x40": (MFCC40, 131),
    "stride10": (["stride10", "stride10_f32"], 67),
    "mfe": (["mfe", "mfe_f32"], 67),
}


@pytest.fixture(scope="module")
def pkg():
    sys.path.insert(0, ROOT)
    import torch  # noqa: F401
    from __graft_entry__ import load_package
    return load_package()


def _blob(name):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from dequantize_model import dequantize
    from continuous_geometry import model_blob
    if name == "synth13":
        return synth_model_blob(**SYNTH13)
    if name in ("stride10", "stride10_f32"):
        return model_blob(name)
    blob = synth_model_blob(**MFE_KW)
    return dequantize(blob) if name == "mfe_f32" else blob


@pytest.fixture(scope="module")
def models(pkg, oracle, tmp_path_factory):
    """name -> (product model, oracle model), created once per module"""
    made = {}
    tmp = tmp_path_factory.mktemp("bank")

    def get(name):
        if name not in made:
            path = os.path.join(MODELS, name)
            if not name.endswith(".kwsm"):
                path = str(tmp / (name + ".kwsm"))
                open(path, "wb").write(_blob(name))
            made[name] = (pkg.Model(path), OracleModel(oracle, path))
        return made[name]

    yield get
    for gm, _ in made.values():
        gm.close()


@pytest.fixture(scope="module")
def banks(pkg, models):
    """bank name -> (Bank, [(product model, oracle model)])"""
    made = {}

    def get(name):
        if name not in made:
            members = [models(n) for n in BANKS[name][0]]
            made[name] = (pkg.Bank([gm for gm, _ in members]), members)
        return made[name]

    yield get
    for bank, _ in made.values():
        bank.close()


@pytest.fixture(scope="module")
def clips(oracle):
    """[n][CLIP] int16: every special clip, then speech-like clips; computed once, never written"""
    sp = np.stack(list(special_clips().values()))
    pcm = np.concatenate([sp, oracle.synth(31, 0, 259 - sp.shape[0])])
    pcm.setflags(write=False)
    return pcm


@pytest.fixture(scope="module")
def references(oracle, models, clips):
    """model name -> (scores, features) of the oracle on the first B clips, computed once per model"""
    made = {}

    def get(name, B):
        if name not in made or made[name][0].shape[0] < B:
            s, f, _ = models(name)[1].run_batch(clips[:B], want_features=True)
            made[name] = (s, f)
        return made[name][0][:B], made[name][1][:B]

    return get


def own_call(gm, d_pcm, B):
    import torch
    s = torch.empty((B, gm.n_labels), dtype=torch.float32, device="cuda")
    f = torch.empty((B, gm.n_features), dtype=torch.float32, device="cuda")
    gm.run_classifier_batch_device(d_pcm.data_ptr(), B, s.data_ptr(), f.data_ptr())
    torch.cuda.synchronize()
    return s.cpu().numpy(), f.cpu().numpy()


def bank_call(bank, d_pcm, B, skip=(), want_features=True, rows=None):
    """([scores per member], features) of one bank call, the buffers sentinel-filled with rows beyond B that the call must leave alone"""
    import torch
    rows = B + 2 if rows is None else rows
    gms = bank.members
    s = [torch.full((rows, gm.n_labels), SENTINEL, dtype=torch.float32, device="cuda") for gm in gms]
    f = torch.full((rows, gms[0].n_features), SENTINEL, dtype=torch.float32, device="cuda")
    bank.run_classifier_batch_device(d_pcm.data_ptr(), B, [None if k in skip else t.data_ptr() for k, t in enumerate(s)],
                                     f.data_ptr() if want_features else None)
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in s], f.cpu().numpy()


@pytest.mark.parametrize("name", list(BANKS))
def test_bank_matches_each_member_and_the_oracle(name, pkg, banks, clips, references):
    import torch
    bank, members = banks(name)
    B = BANKS[name][1]
    assert len(bank) == len(members) and [gm.h.value for gm in bank.members] == [gm.h.value for gm, _ in members]
    kinds = {gm.nn_kernel for gm, _ in members}
    if name == "49x13":
        assert kinds == {"kws_nn_mfma_kernel", "kws_nn_f32_kernel", "kws_nn_kernel"} and B % 4 != 0
    if name == "49x40":
        assert kinds == {"kws_nn_mfma_kernel", "kws_nn_f32_kernel", "kws_nn_kernel"} and [gm.is_float for gm, _ in members] == [False, True, False, True]
    if name == "stride10":
        assert all("lds" in gm.mfcc_kernel or "generic" in gm.mfcc_kernel or "chunked" in gm.mfcc_kernel for gm, _ in members)
    d = torch.from_numpy(clips[:B].copy()).cuda()
    s_bank, f_bank = bank_call(bank, d, B)
    assert (f_bank[B:] == SENTINEL).all()
    for k, (gm, om) in enumerate(members):
        mname = BANKS[name][0][k]
        s_own, f_own = own_call(gm, d, B)
        s_ref, f_ref = references(mname, B)
        s = s_bank[k]
        assert (s[B:] == SENTINEL).all(), mname
        n_bad = int((bits(s[:B]) != bits(s_own)).any(axis=1).sum())
        print("%s / %s (%s): %d of %d clips differ from the member's own call; max |score - oracle| %.3g"
              % (name, mname, gm.nn_kernel, n_bad, B, float(np.abs(s[:B] - s_ref).max())))
        assert n_bad == 0, (name, mname)
        assert (bits(f_bank[:B]) == bits(f_own)).all(), (name, mname)
        assert (bits(f_bank[:B]) == bits(f_ref)).all(), (name, mname)
        if gm.is_float:
            assert np.abs(s[:B] - s_ref).max() <= F32_SCORE_TOL, (name, mname, float(np.abs(s[:B] - s_ref).max()))
        else:
            assert (bits(s[:B]) == bits(s_ref)).all(), (name, mname)
    # without the feature matrix (the bank's own buffer): the same scores
    s2, f2 = bank_call(bank, d, B, want_features=False)
    assert (f2 == SENTINEL).all()
    assert all((bits(a) == bits(b)).all() for a, b in zip(s2, s_bank)), name


def test_bank_subsets_and_sizes(pkg, banks, clips):
    import torch
    bank, members = banks("49x13")
    K = len(members)
    d = torch.from_numpy(clips[:37].copy()).cuda()
    full, f_full = bank_call(bank, d, 37)
    for skip in ({0}, {1}, {2}, {0, 2}, {0, 1, 2}):
        s, f = bank_call(bank, d, 37, skip=skip)
        for k in range(K):
            assert (s[k] == SENTINEL).all() if k in skip else (bits(s[k]) == bits(full[k])).all(), (skip, k)
        assert (bits(f) == bits(f_full)).all(), skip
    # one clip; no clip (nothing written); nothing asked for
    s, f = bank_call(bank, d, 1)
    assert all((bits(s[k][:1]) == bits(full[k][:1])).all() and (s[k][1:] == SENTINEL).all() for k in range(K))
    assert (bits(f[:1]) == bits(f_full[:1])).all() and (f[1:] == SENTINEL).all()
    s, f = bank_call(bank, d, 0)
    assert all((t == SENTINEL).all() for t in s) and (f == SENTINEL).all()
    with pytest.raises(pkg.KwsError) as e:
        bank.run_classifier_batch_device(d.data_ptr(), 37, [None] * K, None)
    assert e.value.code == -20


@pytest.mark.parametrize("name", ["49x13", "49x40", "mfe", "stride10"])
def test_bank_from_cepstra(name, pkg, banks, clips):
    import torch
    bank, members = banks(name)
    B = 45
    d = torch.from_numpy(clips[:B].copy()).cuda()
    gm0 = members[-1][0]                                         # any member's cepstra
    cep = torch.empty((B, gm0.n_features), dtype=torch.float32, device="cuda")
    gm0.mfcc_batch_device(d.data_ptr(), B, cep.data_ptr())
    s = [torch.full((B + 2, gm.n_labels), SENTINEL, dtype=torch.float32, device="cuda") for gm, _ in members]
    f = torch.full((B + 2, gm0.n_features), SENTINEL, dtype=torch.float32, device="cuda")
    bank.cmvn_inference_batch_device(cep.data_ptr(), B, [t.data_ptr() for t in s], f.data_ptr())
    torch.cuda.synchronize()
    for k, (gm, _) in enumerate(members):
        s_own = torch.empty((B, gm.n_labels), dtype=torch.float32, device="cuda")
        f_own = torch.empty((B, gm.n_features), dtype=torch.float32, device="cuda")
        gm.cmvn_inference_batch_device(cep.data_ptr(), B, s_own.data_ptr(), f_own.data_ptr())
        torch.cuda.synchronize()
        got = s[k].cpu().numpy()
        assert (bits(got[:B]) == bits(s_own.cpu().numpy())).all() and (got[B:] == SENTINEL).all(), (name, k)
        assert (bits(f.cpu().numpy()[:B]) == bits(f_own.cpu().numpy())).all(), (name, k)
    assert (f.cpu().numpy()[B:] == SENTINEL).all()


@pytest.mark.parametrize("hop", [1600, 1000])
@pytest.mark.parametrize("name", ["49x13", "49x40", "mfe", "stride10"])
def test_bank_slide(name, hop, pkg, oracle, banks):
    import torch
    bank, members = banks(name)
    recs = [speech(oracle, 41, CLIP + 3 * hop + 7), speech(oracle, 42, CLIP - 1), speech(oracle, 43, 2 * CLIP + 5)]
    offs = np.array([3, 3 + recs[0].size + 11, 3 + recs[0].size + 11 + recs[1].size + 9], np.uint64)
    assert all(int(o) % 2 == 1 for o in offs)
    lens = np.array([r.size for r in recs], np.uint64)
    pcm = np.random.default_rng(5).integers(-30000, 30000, int(offs[-1] + lens[-1]) + 64).astype(np.int16)
    for o, r in zip(offs, recs):
        pcm[int(o):int(o) + r.size] = r
    d = torch.from_numpy(pcm).cuda()
    gm0 = members[0][0]
    n = sum(gm0.slide_window_count(int(x), hop) for x in lens)
    assert n == 4 + 0 + (CLIP + 5) // hop + 1
    stride = gm0.frame_stride_samples                            # 320 samples (8 phases at hop 1000), 160 for the stride-10 ms models (4)
    assert gm0.slide_plan(lens, hop)["phases"] == stride // np.gcd(hop, stride) == (1 if hop == 1600 else 8 if stride == 320 else 4)
    out = {}
    for flags in (AUTO, DIRECT, SHARED):
        s = [torch.full((n + 2, gm.n_labels), SENTINEL, dtype=torch.float32, device="cuda") for gm, _ in members]
        f = torch.full((n + 2, gm0.n_features), SENTINEL, dtype=torch.float32, device="cuda")
        bank.slide_recordings_device(d.data_ptr(), offs, lens, hop, [t.data_ptr() for t in s], f.data_ptr(), flags=flags)
        torch.cuda.synchronize()
        out[flags] = ([t.cpu().numpy() for t in s], f.cpu().numpy())
    for k, (gm, _) in enumerate(members):
        s_own = torch.empty((n, gm.n_labels), dtype=torch.float32, device="cuda")
        f_own = torch.empty((n, gm.n_features), dtype=torch.float32, device="cuda")
        gm.slide_recordings_device(d.data_ptr(), offs, lens, hop, s_own.data_ptr(), f_own.data_ptr())
        torch.cuda.synchronize()
        for flags, (s, f) in out.items():
            assert (bits(s[k][:n]) == bits(s_own.cpu().numpy())).all() and (s[k][n:] == SENTINEL).all(), (name, hop, flags, k)
            assert (bits(f[:n]) == bits(f_own.cpu().numpy())).all() and (f[n:] == SENTINEL).all(), (name, hop, flags, k)
            assert (bits(s[k]) == bits(out[AUTO][0][k])).all() and (bits(f) == bits(out[AUTO][1])).all(), (name, hop, flags, k)
    # no recording long enough for a window: nothing written
    s = [torch.full((2, gm.n_labels), SENTINEL, dtype=torch.float32, device="cuda") for gm, _ in members]
    bank.slide_recordings_device(d.data_ptr(), offs[1:2], lens[1:2], hop, [t.data_ptr() for t in s], None)
    torch.cuda.synchronize()
    assert all((t.cpu().numpy() == SENTINEL).all() for t in s)


def test_bank_leaves_its_members_untouched(pkg, banks, clips):
    """a member in KWS_MODE_FAST with a logits tap: the bank still writes the exact bits, and mode, tap and the member's own results stay"""
    import torch
    bank, members = banks("49x13")
    gm = members[1][0]                                           # the float32 member: fast mode and the tap both apply
    B = 29
    d = torch.from_numpy(clips[:B].copy()).cuda()
    exact, f_exact = bank_call(bank, d, B)
    tap = torch.full((B, gm.n_labels), SENTINEL, dtype=torch.float32, device="cuda")
    gm.set_mode(pkg.MODE_FAST)
    gm.set_logits_tap(tap.data_ptr())
    try:
        s_fast = torch.empty((B, gm.n_labels), dtype=torch.float32, device="cuda")
        gm.run_classifier_batch_device(d.data_ptr(), B, s_fast.data_ptr())
        torch.cuda.synchronize()
        before, tap_before, fb = s_fast.cpu().numpy().copy(), tap.cpu().numpy().copy(), gm.fast_fallback_count()
        assert (tap_before != SENTINEL).all()
        tap.fill_(SENTINEL)
        s, f = bank_call(bank, d, B)
        assert all((bits(a) == bits(b)).all() for a, b in zip(s, exact)) and (bits(f) == bits(f_exact)).all()
        assert (tap.cpu().numpy() == SENTINEL).all(), "a bank call wrote a member's logits tap"
        assert gm.L.kws_get_mode(gm.h) == pkg.MODE_FAST and gm.fast_fallback_count() == fb
        gm.run_classifier_batch_device(d.data_ptr(), B, s_fast.data_ptr())
        torch.cuda.synchronize()
        assert (bits(s_fast.cpu().numpy()) == bits(before)).all() and (bits(tap.cpu().numpy()) == bits(tap_before)).all()
    finally:
        gm.set_logits_tap(None)
        gm.set_mode(pkg.MODE_EXACT)


def test_bank_refusals_and_stream_ordering(pkg, models, banks, clips):
    import torch
    l476, l432 = models("l476_no_yes.kwsm")[0], models("l432_trick_or_treat.kwsm")[0]
    with pytest.raises(pkg.KwsError) as e:
        pkg.Bank([l476, l432])
    assert e.value.code == -20 and "high_frequency" in str(e.value)
    for bad in ([], [l476, l476], [l476] * 17):
        with pytest.raises(pkg.KwsError) as e:
            pkg.Bank(bad)
        assert e.value.code == -20
    # a member's own call on another stream, then the bank on the default stream, reading what that call leaves in the member's scratch
    # class: the bank call must wait for it and both results must be right
    bank, members = banks("49x13")
    B = 259
    d = torch.from_numpy(clips[:B].copy()).cuda()
    exact, _ = bank_call(bank, d, B)
    gm = members[2][0]                                           # the generic int8 member: its int8 tensor lives in the handle's scratch
    own, _ = own_call(gm, d, B)
    side = torch.cuda.Stream()
    s_side = torch.empty((B, gm.n_labels), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    gm.run_classifier_batch_device(d.data_ptr(), B, s_side.data_ptr(), stream=side.cuda_stream)
    s, _ = bank_call(bank, d, B)
    torch.cuda.synchronize()
    assert (bits(s_side.cpu().numpy()) == bits(own)).all()
    assert all((bits(a) == bits(b)).all() for a, b in zip(s, exact))
