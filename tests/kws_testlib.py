"""ctypes bindings used by the tests: the C oracle (oracle/libkws_oracle.so), the compiled
reference (oracle/_ref/libei_ref_l476.so, only where it has been built) and small helpers.

Test infrastructure only -- nothing here is imported by the product package.
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# KWS_ORACLE_SO: another build of oracle/kws_oracle.c (tests/test_sanitizers.py points it at the ASan + UBSan build)
ORACLE_SO = os.environ.get("KWS_ORACLE_SO") or os.path.join(ROOT, "oracle", "libkws_oracle.so")
REF_SO = os.path.join(ROOT, "oracle", "_ref", "libei_ref_l476.so")
REF_QFB_SO = os.path.join(ROOT, "oracle", "_ref", "libei_ref_l476_qfb.so")      # the same sources with EIDSP_QUANTIZE_FILTERBANK at the SDK's default (1)
MODELS = os.path.join(ROOT, "models")
GOLDEN = os.path.join(ROOT, "tests", "golden")
CLIP_LEN = 16000


class MfccConfig(C.Structure):
    _fields_ = [("num_cepstral", C.c_int), ("frame_length", C.c_float), ("frame_stride", C.c_float),
                ("num_filters", C.c_int), ("fft_length", C.c_int), ("win_size", C.c_int),
                ("low_frequency", C.c_int), ("high_frequency", C.c_int), ("pre_cof", C.c_float),
                ("pre_shift", C.c_int), ("sampling_frequency", C.c_int), ("quantize_filterbank", C.c_int)]

    def copy(self, **kw):
        c = MfccConfig()
        for f, _ in self._fields_:
            setattr(c, f, kw.get(f, getattr(self, f)))
        return c


def L476_CONFIG():
    return MfccConfig(13, 0.02, 0.02, 32, 256, 101, 300, 4000, 0.98, 1, 16000)


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def build_oracle():
    if not os.path.exists(ORACLE_SO) or os.path.getmtime(ORACLE_SO) < os.path.getmtime(
            os.path.join(ROOT, "oracle", "kws_oracle.c")):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "oracle"), "oracle"])


class Oracle:
    """The plain-C restatement (oracle/kws_oracle.c)."""

    def __init__(self):
        build_oracle()
        L = self.L = C.CDLL(ORACLE_SO)
        L.kwso_log.restype = C.c_float
        L.kwso_log.argtypes = [C.c_float]
        L.kwso_frequency_to_mel.restype = C.c_float
        L.kwso_frequency_to_mel.argtypes = [C.c_float]
        L.kwso_mel_to_frequency.restype = C.c_float
        L.kwso_mel_to_frequency.argtypes = [C.c_float]
        L.kwso_num_frames.argtypes = [C.c_size_t, C.POINTER(MfccConfig)]
        L.kwso_filterbanks.argtypes = [C.POINTER(MfccConfig), C.c_void_p]
        L.kwso_preemphasis.argtypes = [C.c_void_p, C.c_size_t, C.c_float, C.c_int, C.c_size_t, C.c_size_t, C.c_void_p]
        L.kwso_rfft_complex.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        L.kwso_power_spectrum.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_int]
        L.kwso_mfe.argtypes = [C.c_void_p, C.c_size_t, C.POINTER(MfccConfig), C.c_void_p, C.c_void_p]
        L.kwso_dct2_ortho.argtypes = [C.c_void_p, C.c_int]
        L.kwso_mfcc_nocmvn.argtypes = [C.c_void_p, C.c_size_t, C.POINTER(MfccConfig), C.c_void_p]
        L.kwso_cmvnw.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int]
        L.kwso_cmvnw_scale.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]
        L.kwso_extract_mfe.argtypes = [C.c_void_p, C.c_size_t, C.POINTER(MfccConfig), C.c_void_p]
        L.kwso_normalize.argtypes = [C.c_void_p, C.c_size_t]
        L.kwso_extract_mfcc.argtypes = [C.c_void_p, C.c_size_t, C.POINTER(MfccConfig), C.c_void_p]
        L.kwso_srdhm.restype = C.c_int32
        L.kwso_srdhm.argtypes = [C.c_int32, C.c_int32]
        L.kwso_rdivpot.restype = C.c_int32
        L.kwso_rdivpot.argtypes = [C.c_int32, C.c_int]
        L.kwso_mbqm.restype = C.c_int32
        L.kwso_mbqm.argtypes = [C.c_int32, C.c_int32, C.c_int]
        L.kwso_quantize_multiplier.argtypes = [C.c_double, C.POINTER(C.c_int32), C.POINTER(C.c_int)]
        L.kwso_exp_on_negative_values_q5_26.restype = C.c_int32
        L.kwso_exp_on_negative_values_q5_26.argtypes = [C.c_int32]
        L.kwso_one_over_one_plus_x.restype = C.c_int32
        L.kwso_one_over_one_plus_x.argtypes = [C.c_int32]
        L.kwso_model_load.restype = C.c_void_p
        L.kwso_model_load.argtypes = [C.c_void_p, C.c_size_t]
        L.kwso_model_free.argtypes = [C.c_void_p]
        for f in ("label_count", "feature_count", "raw_sample_count", "tensor_count", "dsp_block"):
            getattr(L, "kwso_model_" + f).argtypes = [C.c_void_p]
        L.kwso_model_label.restype = C.c_char_p
        L.kwso_model_label.argtypes = [C.c_void_p, C.c_int]
        L.kwso_model_tensor_bytes.argtypes = [C.c_void_p, C.c_int]
        L.kwso_model_mfcc_config.argtypes = [C.c_void_p, C.POINTER(MfccConfig)]
        L.kwso_quantize_input.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.kwso_nn_invoke.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.kwso_dequantize_output.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.kwso_run_inference.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.kwso_run_classifier.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
        L.kwso_run_classifier_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p,
                                                C.c_void_p, C.c_void_p]
        L.kwso_time_run_classifier.restype = C.c_double
        L.kwso_time_run_classifier.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_int, C.c_void_p]
        L.kwso_synth_fill.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p]
        L.kwso_mix_audio.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_float, C.c_float, C.c_int, C.c_void_p]
        L.kwso_model_is_float.argtypes = [C.c_void_p]
        L.kwso_nn_invoke_f32.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.kwso_continuous_create.restype = C.c_void_p
        L.kwso_continuous_create.argtypes = [C.c_void_p]
        L.kwso_continuous_free.argtypes = [C.c_void_p]
        L.kwso_continuous_init.argtypes = [C.c_void_p]
        L.kwso_continuous_step.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.POINTER(C.c_int)]
        L.kwso_continuous_step_ex.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p, C.c_void_p, C.POINTER(C.c_int)]

    def mix_audio(self, word, noise_window, word_vol, bg_vol, n):
        """mix_audio of dataset-curation.py:93-137 (PARITY UNPINNED, see oracle/kws_oracle.h); word / noise_window may be None"""
        out = np.zeros(n, np.int16)
        w = None if word is None else np.ascontiguousarray(word, np.float32)
        b = None if noise_window is None else np.ascontiguousarray(noise_window, np.float32)
        self.L.kwso_mix_audio(None if w is None else _ptr(w), 0 if w is None else w.size, None if b is None else _ptr(b), word_vol, bg_vol, n, _ptr(out))
        return out

    # ---- clips
    def synth(self, seed, first, n, clip_len=CLIP_LEN):
        out = np.empty((n, clip_len), np.int16)
        self.L.kwso_synth_fill(seed, first, n, clip_len, _ptr(out))
        return out

    # ---- DSP
    def num_frames(self, n, cfg):
        return self.L.kwso_num_frames(n, C.byref(cfg))

    def quantize_zero_one(self, v):
        self.L.kwso_quantize_zero_one.restype = C.c_float
        self.L.kwso_quantize_zero_one.argtypes = [C.c_float]
        return self.L.kwso_quantize_zero_one(float(v))

    def filterbanks(self, cfg):
        out = np.zeros((cfg.fft_length // 2 + 1, cfg.num_filters), np.float32)
        rc = self.L.kwso_filterbanks(C.byref(cfg), _ptr(out))
        assert rc == 0, rc
        return out

    def preemphasis(self, pcm, cof, shift, offset, length):
        pcm = np.ascontiguousarray(pcm, np.int16)
        out = np.zeros(length, np.float32)
        rc = self.L.kwso_preemphasis(_ptr(pcm), pcm.size, cof, shift, offset, length, _ptr(out))
        assert rc == 0, rc
        return out

    def rfft_complex(self, x):
        x = np.ascontiguousarray(x, np.float32)
        out = np.zeros((x.size // 2 + 1, 2), np.float32)
        rc = self.L.kwso_rfft_complex(_ptr(x), x.size, _ptr(out))
        assert rc == 0, rc
        return out

    def power_spectrum(self, frame, fft_length):
        frame = np.ascontiguousarray(frame, np.float32)
        out = np.zeros(fft_length // 2 + 1, np.float32)
        rc = self.L.kwso_power_spectrum(_ptr(frame), frame.size, _ptr(out), fft_length)
        assert rc == 0, rc
        return out

    def mfe(self, pcm, cfg):
        pcm = np.ascontiguousarray(pcm, np.int16)
        nf = self.num_frames(pcm.size, cfg)
        feat = np.zeros((nf, cfg.num_filters), np.float32)
        en = np.zeros(nf, np.float32)
        rc = self.L.kwso_mfe(_ptr(pcm), pcm.size, C.byref(cfg), _ptr(feat), _ptr(en))
        assert rc == 0, rc
        return feat, en

    def dct2_ortho(self, v):
        v = np.array(v, np.float32)
        rc = self.L.kwso_dct2_ortho(_ptr(v), v.size)
        assert rc == 0, rc
        return v

    def mfcc_nocmvn(self, pcm, cfg):
        pcm = np.ascontiguousarray(pcm, np.int16)
        nf = self.num_frames(pcm.size, cfg)
        out = np.zeros((nf, cfg.num_cepstral), np.float32)
        rc = self.L.kwso_mfcc_nocmvn(_ptr(pcm), pcm.size, C.byref(cfg), _ptr(out))
        assert rc == 0, rc
        return out

    def cmvnw(self, m, win_size, var_norm=True):
        m = np.array(m, np.float32)
        rc = self.L.kwso_cmvnw(_ptr(m), m.shape[0], m.shape[1], win_size, int(var_norm))
        assert rc == 0, rc
        return m

    def cmvnw_scale(self, m, win_size, var_norm=False, scale=True):
        """L432 SDK copy: processing::cmvnw(matrix, win_size, variance_normalization, scale)."""
        m = np.array(m, np.float32)
        rc = self.L.kwso_cmvnw_scale(_ptr(m), m.shape[0], m.shape[1], win_size, int(var_norm), int(scale))
        assert rc == 0, rc
        return m

    def extract_mfe(self, pcm, cfg):
        """L432 SDK copy: extract_mfe_features (no pre-emphasis whatever cfg.pre_cof says)."""
        pcm = np.ascontiguousarray(pcm, np.int16)
        c = MfccConfig.from_buffer_copy(cfg)
        c.pre_cof = 0.0
        nf = self.num_frames(pcm.size, c)
        out = np.zeros(nf * c.num_filters, np.float32)
        rc = self.L.kwso_extract_mfe(_ptr(pcm), pcm.size, C.byref(c), _ptr(out))
        assert rc == 0, rc
        return out

    def extract_mfcc(self, pcm, cfg):
        pcm = np.ascontiguousarray(pcm, np.int16)
        nf = self.num_frames(pcm.size, cfg)
        out = np.zeros(nf * cfg.num_cepstral, np.float32)
        rc = self.L.kwso_extract_mfcc(_ptr(pcm), pcm.size, C.byref(cfg), _ptr(out))
        assert rc == 0, rc
        return out

    def quantize_multiplier(self, m):
        q, s = C.c_int32(), C.c_int()
        self.L.kwso_quantize_multiplier(m, C.byref(q), C.byref(s))
        return q.value, s.value


class OracleModel:
    def __init__(self, oracle, path):
        self.o = oracle
        self.blob = open(path, "rb").read()
        self.h = oracle.L.kwso_model_load(self.blob, len(self.blob))
        assert self.h, "kwso_model_load failed for %s" % path
        L = oracle.L
        self.n_labels = L.kwso_model_label_count(self.h)
        self.labels = [L.kwso_model_label(self.h, i).decode() for i in range(self.n_labels)]
        self.n_features = L.kwso_model_feature_count(self.h)
        self.raw_sample_count = L.kwso_model_raw_sample_count(self.h)
        self.cfg = MfccConfig()
        L.kwso_model_mfcc_config(self.h, C.byref(self.cfg))
        self.tensor_bytes = [L.kwso_model_tensor_bytes(self.h, i) for i in range(L.kwso_model_tensor_count(self.h))]

    def quantize_input(self, feat):
        feat = np.ascontiguousarray(feat, np.float32)
        q = np.zeros(self.n_features, np.int8)
        self.o.L.kwso_quantize_input(self.h, _ptr(feat), _ptr(q))
        return q

    def nn_invoke(self, q, taps=False):
        q = np.ascontiguousarray(q, np.int8)
        out = np.zeros(self.n_labels, np.int8)
        tp = np.zeros(sum(self.tensor_bytes), np.int8) if taps else None
        rc = self.o.L.kwso_nn_invoke(self.h, _ptr(q), _ptr(out), _ptr(tp) if taps else None)
        assert rc == 0, rc
        if not taps:
            return out
        offs = np.cumsum([0] + self.tensor_bytes)
        return out, [tp[offs[i]:offs[i + 1]] for i in range(len(self.tensor_bytes))]

    def nn_invoke_f32(self, feat, taps=False):
        """float graph; taps -> list of float32 arrays, one per tensor (tensor-id order)"""
        feat = np.ascontiguousarray(feat, np.float32)
        out = np.zeros(self.n_labels, np.float32)
        tp = np.zeros(sum(self.tensor_bytes) // 4 + 1, np.float32) if taps else None
        rc = self.o.L.kwso_nn_invoke_f32(self.h, _ptr(feat), _ptr(out), _ptr(tp) if taps else None)
        assert rc == 0, rc
        if not taps:
            return out
        offs = np.cumsum([0] + [b // 4 for b in self.tensor_bytes])
        return out, [tp[offs[i]:offs[i + 1]] for i in range(len(self.tensor_bytes))]

    def dequantize(self, out_q):
        out_q = np.ascontiguousarray(out_q, np.int8)
        s = np.zeros(self.n_labels, np.float32)
        self.o.L.kwso_dequantize_output(self.h, _ptr(out_q), _ptr(s))
        return s

    def run_inference(self, feat):
        feat = np.ascontiguousarray(feat, np.float32)
        s = np.zeros(self.n_labels, np.float32)
        rc = self.o.L.kwso_run_inference(self.h, _ptr(feat), _ptr(s))
        assert rc == 0, rc
        return s

    def run_batch(self, pcm, want_features=False):
        pcm = np.ascontiguousarray(pcm, np.int16)
        if pcm.ndim == 1:
            pcm = pcm[None]
        B, n = pcm.shape
        s = np.zeros((B, self.n_labels), np.float32)
        f = np.zeros((B, self.n_features), np.float32)
        q = np.zeros((B, self.n_features), np.int8)
        rc = self.o.L.kwso_run_classifier_batch(self.h, _ptr(pcm), n, B, _ptr(s), _ptr(f), _ptr(q))
        if rc != 0:
            return rc
        return (s, f, q) if want_features else s

    def time_run(self, pcm, iters=1):
        pcm = np.ascontiguousarray(pcm, np.int16)
        chk = C.c_float()
        return self.o.L.kwso_time_run_classifier(self.h, _ptr(pcm), pcm.shape[0], pcm.shape[1], iters, C.byref(chk))


class OracleContinuous:
    """run_classifier_init / run_classifier_continuous restated (oracle/kws_oracle.c)."""

    def __init__(self, model):
        self.m = model
        self.L = model.o.L
        self.h = self.L.kwso_continuous_create(model.h)
        assert self.h

    def init(self):
        self.L.kwso_continuous_init(self.h)

    def step(self, slice_pcm):
        slice_pcm = np.ascontiguousarray(slice_pcm, np.int16)
        s = np.zeros(self.m.n_labels, np.float32)
        produced = C.c_int()
        rc = self.L.kwso_continuous_step(self.h, _ptr(slice_pcm), slice_pcm.size, None, _ptr(s), C.byref(produced))
        return rc, bool(produced.value), s


def have_reference():
    return os.path.exists(REF_SO)


REF432_SO = os.path.join(ROOT, "oracle", "_ref", "libei_ref_l432dsp.so")


class ReferenceL432Dsp:
    """processing.hpp + numpy.hpp of the L432 SDK copy, compiled in place (oracle/ref_l432_dsp.cpp)."""

    def __init__(self):
        L = self.L = C.CDLL(REF432_SO)
        L.eiref432_cmvnw.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]
        L.eiref432_normalize.argtypes = [C.c_void_p, C.c_int, C.c_int]

    def cmvnw(self, m, win_size, var_norm, scale):
        m = np.array(m, np.float32)
        rc = self.L.eiref432_cmvnw(_ptr(m), m.shape[0], m.shape[1], win_size, int(var_norm), int(scale))
        assert rc == 0, rc
        return m

    def normalize(self, m):
        m = np.array(m, np.float32)
        rc = self.L.eiref432_normalize(_ptr(m), m.shape[0], m.shape[1])
        assert rc == 0, rc
        return m


class Reference:
    """The unmodified reference SDK compiled by oracle/Makefile (target ref).  qfb: the build with EIDSP_QUANTIZE_FILTERBANK = 1."""

    def __init__(self, qfb=False):
        L = self.L = C.CDLL(REF_QFB_SO if qfb else REF_SO)
        assert L.eiref_quantize_filterbank() == (1 if qfb else 0)
        L.eiref_quantize_zero_one.restype = C.c_float
        L.eiref_quantize_zero_one.argtypes = [C.c_float]
        L.eiref_quantized_table.argtypes = [C.c_void_p, C.c_int]
        L.eiref_label.restype = C.c_char_p
        L.eiref_run_classifier.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p]
        L.eiref_extract_mfcc.argtypes = [C.c_void_p, C.c_size_t, C.c_int, C.c_float, C.c_float, C.c_int, C.c_int,
                                         C.c_int, C.c_int, C.c_int, C.c_float, C.c_int, C.c_void_p, C.c_size_t]
        L.eiref_mfcc_nocmvn.argtypes = [C.c_void_p, C.c_size_t, C.c_int, C.c_float, C.c_float, C.c_int, C.c_int,
                                        C.c_int, C.c_int, C.c_float, C.c_int, C.c_void_p]
        L.eiref_mfe.argtypes = [C.c_void_p, C.c_size_t, C.c_float, C.c_float, C.c_int, C.c_int, C.c_int, C.c_int,
                                C.c_float, C.c_int, C.c_void_p, C.c_void_p]
        L.eiref_preemphasis.argtypes = [C.c_void_p, C.c_size_t, C.c_float, C.c_int, C.c_size_t, C.c_size_t, C.c_void_p]
        L.eiref_power_spectrum.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_int]
        L.eiref_filterbanks.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]
        L.eiref_log.restype = C.c_float
        L.eiref_log.argtypes = [C.c_float]
        L.eiref_frequency_to_mel.restype = C.c_float
        L.eiref_frequency_to_mel.argtypes = [C.c_float]
        L.eiref_mel_to_frequency.restype = C.c_float
        L.eiref_mel_to_frequency.argtypes = [C.c_float]
        L.eiref_dct2_ortho.argtypes = [C.c_void_p, C.c_size_t]
        L.eiref_cmvnw.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int]
        L.eiref_num_frames.argtypes = [C.c_size_t, C.c_float, C.c_float]
        L.eiref_rfft_complex.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p]
        L.eiref_run_inference.argtypes = [C.c_void_p, C.c_void_p]
        L.eiref_nn_taps.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        L.eiref_continuous.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.POINTER(C.c_int), C.c_void_p]
        L.eiref_time_run_classifier.restype = C.c_double
        L.eiref_time_run_classifier.argtypes = [C.c_void_p, C.c_size_t, C.c_size_t, C.c_int, C.c_void_p]
        L.eiref_graph_run.argtypes = [C.c_char_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p]
        L.eiref_time_graph_classifier.restype = C.c_double
        L.eiref_time_graph_classifier.argtypes = [C.c_char_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_size_t, C.c_int, C.c_void_p]
        self.n_labels = L.eiref_label_count()
        self.labels = [L.eiref_label(i).decode() for i in range(self.n_labels)]
        self.n_features = L.eiref_feature_count()
        self.tensor_bytes = [L.eiref_tensor_bytes(i) for i in range(L.eiref_tensor_count())]

    def graph_run(self, blob, x):
        """A .kwsm graph through the reference's own TFLite-Micro op registrations (init/prepare/invoke).
        x: the input tensor (int8 or float32).  Returns (output, [every tensor as raw bytes, tensor-id order])."""
        import eon_import
        tens, _, t_in, t_out, _ = eon_import.parse_blob(blob)
        x = np.ascontiguousarray(x)
        np_t = {1: np.float32, 2: np.int32, 9: np.int8}
        out = np.zeros(tens[t_out]["nbytes"] // np.dtype(np_t[tens[t_out]["type"]]).itemsize, np_t[tens[t_out]["type"]])
        taps = np.zeros(sum(t["nbytes"] for t in tens), np.uint8)
        rc = self.L.eiref_graph_run(blob, len(blob), _ptr(x), x.nbytes, _ptr(out), out.nbytes, _ptr(taps))
        assert rc == 0, rc
        offs = np.cumsum([0] + [t["nbytes"] for t in tens])
        return out, [taps[offs[i]:offs[i + 1]].view(np_t[t["type"]]) for i, t in enumerate(tens)]

    def time_graph(self, blob, pcm, iters=1):
        """seconds for iters passes of extract_mfcc_features + the blob's graph (reference op code) over pcm [n][len]"""
        pcm = np.ascontiguousarray(pcm, np.int16)
        chk = C.c_float()
        t = self.L.eiref_time_graph_classifier(blob, len(blob), _ptr(pcm), pcm.shape[0], pcm.shape[1], iters, C.byref(chk))
        assert t >= 0, t
        return t

    # ---- boundary behaviour (debug text, the cancellation hook): oracle/ref_driver.cpp eiref_*_full -------------------------
    def boundary_call(self, kind, data, debug=False, cancel_at=0):
        """kind: 'oneshot' (int16 window) | 'inference' (float features) | 'continuous' (int16 slice).  Returns (rc, polls of the
        cancellation hook, the caller's ei_impulse_result_t byte for byte -- pre-filled with 0xA5 --, label flags, printed text)."""
        L = self.L
        L.eiref_capture.argtypes = [C.c_void_p, C.c_size_t]
        L.eiref_capture_len.restype = C.c_size_t
        fn = {"oneshot": L.eiref_run_classifier_full, "inference": L.eiref_run_inference_full, "continuous": L.eiref_continuous_full}[kind]
        buf = C.create_string_buffer(1 << 16)
        res = np.zeros(L.eiref_result_size(), np.uint8)
        lab = np.zeros(self.n_labels, np.int32)
        L.eiref_capture(buf, len(buf))
        L.eiref_cancel_at(int(cancel_at))
        if kind == "inference":
            x = np.ascontiguousarray(data, np.float32)
            fn.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
            rc = fn(_ptr(x), int(debug), _ptr(res), _ptr(lab))
        else:
            x = np.ascontiguousarray(data, np.int16)
            fn.argtypes = [C.c_void_p, C.c_size_t, C.c_int, C.c_void_p, C.c_void_p]
            rc = fn(_ptr(x), x.size, int(debug), _ptr(res), _ptr(lab))
        n = L.eiref_capture_len()
        polls = L.eiref_cancel_polls()
        L.eiref_capture(None, 0)
        L.eiref_cancel_at(0)
        return rc, polls, res, lab, buf.raw[:n]

    def run_classifier(self, pcm):
        pcm = np.ascontiguousarray(pcm, np.int16)
        s = np.zeros(self.n_labels, np.float32)
        tl, gc = C.c_size_t(), C.c_size_t()
        rc = self.L.eiref_run_classifier(_ptr(pcm), pcm.size, _ptr(s), C.byref(tl), C.byref(gc))
        return rc, s, tl.value, gc.value

    def _cfg_args(self, cfg, with_win):
        a = [cfg.num_cepstral, cfg.frame_length, cfg.frame_stride, cfg.num_filters, cfg.fft_length]
        if with_win:
            a.append(cfg.win_size)
        return a + [cfg.low_frequency, cfg.high_frequency, cfg.pre_cof, cfg.pre_shift]

    def num_frames(self, n, cfg):
        return self.L.eiref_num_frames(n, cfg.frame_length, cfg.frame_stride)

    def extract_mfcc(self, pcm, cfg):
        pcm = np.ascontiguousarray(pcm, np.int16)
        nf = self.num_frames(pcm.size, cfg)
        out = np.zeros(nf * cfg.num_cepstral, np.float32)
        rc = self.L.eiref_extract_mfcc(_ptr(pcm), pcm.size, *self._cfg_args(cfg, True), _ptr(out), out.size)
        assert rc == 0, rc
        return out

    def mfcc_nocmvn(self, pcm, cfg):
        pcm = np.ascontiguousarray(pcm, np.int16)
        nf = self.num_frames(pcm.size, cfg)
        out = np.zeros((nf, cfg.num_cepstral), np.float32)
        rc = self.L.eiref_mfcc_nocmvn(_ptr(pcm), pcm.size, *self._cfg_args(cfg, False), _ptr(out))
        assert rc == 0, rc
        return out

    def mfe(self, pcm, cfg):
        pcm = np.ascontiguousarray(pcm, np.int16)
        nf = self.num_frames(pcm.size, cfg)
        feat = np.zeros((nf, cfg.num_filters), np.float32)
        en = np.zeros(nf, np.float32)
        rc = self.L.eiref_mfe(_ptr(pcm), pcm.size, cfg.frame_length, cfg.frame_stride, cfg.num_filters,
                              cfg.fft_length, cfg.low_frequency, cfg.high_frequency, cfg.pre_cof, cfg.pre_shift,
                              _ptr(feat), _ptr(en))
        assert rc == 0, rc
        return feat, en

    def preemphasis(self, pcm, cof, shift, offset, length):
        pcm = np.ascontiguousarray(pcm, np.int16)
        out = np.zeros(length, np.float32)
        rc = self.L.eiref_preemphasis(_ptr(pcm), pcm.size, cof, shift, offset, length, _ptr(out))
        assert rc == 0, rc
        return out

    def power_spectrum(self, frame, fft_length):
        frame = np.array(frame, np.float32)
        out = np.zeros(fft_length // 2 + 1, np.float32)
        rc = self.L.eiref_power_spectrum(_ptr(frame), frame.size, _ptr(out), fft_length)
        assert rc == 0, rc
        return out

    def filterbanks(self, cfg):
        out = np.zeros((cfg.fft_length // 2 + 1, cfg.num_filters), np.float32)
        hf = cfg.high_frequency if cfg.high_frequency else cfg.sampling_frequency // 2
        rc = self.L.eiref_filterbanks(cfg.num_filters, cfg.fft_length, cfg.low_frequency, hf, _ptr(out))
        assert rc == 0, rc
        return out

    def rfft_complex(self, x):
        x = np.ascontiguousarray(x, np.float32)
        out = np.zeros((x.size // 2 + 1, 2), np.float32)
        rc = self.L.eiref_rfft_complex(_ptr(x), x.size, _ptr(out))
        assert rc == 0, rc
        return out

    def dct2_ortho(self, v):
        v = np.array(v, np.float32)
        rc = self.L.eiref_dct2_ortho(_ptr(v), v.size)
        assert rc == 0, rc
        return v

    def cmvnw(self, m, win_size, var_norm=True):
        m = np.array(m, np.float32)
        rc = self.L.eiref_cmvnw(_ptr(m), m.shape[0], m.shape[1], win_size, int(var_norm))
        assert rc == 0, rc
        return m

    def run_inference(self, feat):
        feat = np.ascontiguousarray(feat, np.float32)
        s = np.zeros(self.n_labels, np.float32)
        rc = self.L.eiref_run_inference(_ptr(feat), _ptr(s))
        assert rc == 0, rc
        return s

    def nn_taps(self, q):
        """all op outputs (tensor id -> bytes) of the int8 graph for input tensor q"""
        q = np.ascontiguousarray(q, np.int8)
        ids = np.arange(len(self.tensor_bytes), dtype=np.int32)
        out = np.zeros(sum(self.tensor_bytes), np.int8)
        sizes = np.zeros(ids.size, np.int32)
        rc = self.L.eiref_nn_taps(_ptr(q), ids.size, _ptr(ids), _ptr(out), _ptr(sizes))
        assert rc == 0, rc
        offs = np.cumsum([0] + self.tensor_bytes)
        return {int(i): out[offs[i]:offs[i + 1]].copy() for i in ids if sizes[i] >= 0}

    def traced(self, fn, *args, cap=4096):
        """fn(*args) with every get_data call the reference makes recorded: (result of fn, int64 [n_calls, 3] = offset, length, return value)."""
        buf = np.zeros((cap, 3), np.int64)
        self.L.eiref_trace_get_data.argtypes = [C.c_void_p, C.c_int]
        self.L.eiref_trace_get_data(_ptr(buf), cap)
        try:
            out = fn(*args)
            n = self.L.eiref_trace_count()
        finally:
            self.L.eiref_trace_get_data(None, 0)
        assert n <= cap, n
        return out, buf[:n].copy()

    def continuous_init(self):
        self.L.eiref_continuous_init()

    def continuous(self, slice_pcm):
        slice_pcm = np.ascontiguousarray(slice_pcm, np.int16)
        s = np.zeros(self.n_labels, np.float32)
        produced = C.c_int()
        tl = C.c_size_t()
        rc = self.L.eiref_continuous(_ptr(slice_pcm), slice_pcm.size, _ptr(s), C.byref(produced), C.byref(tl))
        return rc, bool(produced.value), s, tl.value

    def time_run(self, pcm, iters=1):
        pcm = np.ascontiguousarray(pcm, np.int16)
        chk = C.c_float()
        return self.L.eiref_time_run_classifier(_ptr(pcm), pcm.shape[0], pcm.shape[1], iters, C.byref(chk))


def reference_float_twin(reference, tensors, feat):
    """Run the fp32 twin of the shipped graph through the REFERENCE's float TFLite-Micro kernels,
    called leaf by leaf (oracle/ref_driver.cpp eiref_f32_*).  tensors: constant tensors of the .kwsm (id -> float array).
    Returns (logits[4], scores[4])."""
    L = reference.L
    fp = C.POINTER(C.c_float)
    FLT_MAX = float(np.finfo(np.float32).max)

    def P(a):
        return a.ctypes.data_as(fp)

    def F(x):
        return C.c_float(x)

    x = np.ascontiguousarray(feat, np.float32)
    y1 = np.zeros(49 * 30, np.float32)
    L.eiref_f32_conv(P(x), 1, 49, 13, P(tensors[7]), 30, 1, 7, P(tensors[6]), 3, 0, F(-FLT_MAX), F(FLT_MAX), P(y1), 1, 49)
    y2 = np.zeros(49 * 30, np.float32)
    L.eiref_f32_add_bcast(P(y1), (C.c_int * 4)(1, 1, 49, 30), P(tensors[2]), (C.c_int * 4)(1, 1, 1, 30),
                          (C.c_int * 4)(1, 1, 49, 30), F(0.0), F(FLT_MAX), P(y2))
    y3 = np.zeros(7 * 30, np.float32)
    L.eiref_f32_maxpool(P(y2), 49, 1, 30, 7, 1, 7, 1, F(-FLT_MAX), F(FLT_MAX), P(y3), 7, 1)
    y4 = np.zeros(70, np.float32)
    L.eiref_f32_conv(P(y3), 1, 7, 30, P(tensors[9]), 10, 1, 7, P(tensors[8]), 3, 0, F(-FLT_MAX), F(FLT_MAX), P(y4), 1, 7)
    y5 = np.zeros(70, np.float32)
    L.eiref_f32_add_bcast(P(y4), (C.c_int * 4)(1, 1, 7, 10), P(tensors[3]), (C.c_int * 4)(1, 1, 1, 10),
                          (C.c_int * 4)(1, 1, 7, 10), F(0.0), F(FLT_MAX), P(y5))
    y6 = np.zeros(10, np.float32)
    L.eiref_f32_maxpool(P(y5), 7, 1, 10, 7, 1, 7, 1, F(-FLT_MAX), F(FLT_MAX), P(y6), 1, 1)
    lg = np.zeros(4, np.float32)
    L.eiref_f32_fc(P(y6), 10, P(tensors[5]), 4, P(tensors[4]), F(-FLT_MAX), F(FLT_MAX), P(lg))
    sc = np.zeros(4, np.float32)
    L.eiref_f32_softmax(P(lg), 4, F(1.0), P(sc))
    return lg, sc


def bits(a):
    """view float32 array as uint32 for exact comparison"""
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def special_clips():
    """known-answer / edge-case clips"""
    z = np.zeros(CLIP_LEN, np.int16)
    alt = np.empty(CLIP_LEN, np.int16)
    alt[0::2] = 32767
    alt[1::2] = -32767
    step = np.zeros(CLIP_LEN, np.int16)
    step[8000:] = 20000
    imp = np.zeros(CLIP_LEN, np.int16)
    imp[5000] = 32767
    imp[15999] = -32768
    mn = np.full(CLIP_LEN, -32768, np.int16)
    ramp = (np.arange(CLIP_LEN) * 4 - 32000).astype(np.int16)
    return {"zeros": z, "alternating_fullscale": alt, "step": step, "impulses": imp, "min": mn, "ramp": ramp}


# ---------------------------------------------------------------------------------------------------------------
#  synthetic models of the Edge Impulse 1-D CNN family (random weights / quantisation): tools/synth_model.py
# ---------------------------------------------------------------------------------------------------------------
sys.path.insert(0, os.path.join(ROOT, "tools"))
from synth_model import synth_model_blob  # noqa: E402,F401

# Named synthetic graphs shared by the CPU pins (oracle vs the reference's op registrations), tools/make_golden.py and
# the GPU parity tests.  `dw` / `pw` blocks: DEPTHWISE_CONV_2D / pointwise CONV_2D (BASELINE config 5).
SYNTH_SPECS = {
    "seed1": dict(seed=1),                                                                # shipped shape, random weights
    "seed2": dict(seed=2, ncep=10, win_size=51, high=0, blocks=((16, 5, 7), (8, 3, 7)), n_labels=3),
    "seed4": dict(seed=4, ncep=16, blocks=((32, 8, 7), (16, 8, 7)), n_labels=5, add_bias=False),   # matrix-core limits, even taps
    "seed5": dict(seed=5, ncep=13, blocks=((30, 7, 7), (10, 7, 7)), n_labels=4, conv_bias=True),
    "seed6": dict(seed=6, ncep=12, win_size=13, low=0, high=8000, blocks=((20, 3, 7), (12, 5, 1), (6, 3, 7)), n_labels=2),  # 3 blocks
    "seed7": dict(seed=7, ncep=13, blocks=((40, 7, 7), (10, 7, 7)), n_labels=4),           # 40 channels
    "f40c40": dict(seed=11, num_filters=40, ncep=40, low=300, high=0, blocks=((16, 5, 7), (8, 3, 7)), n_labels=3),
    "dscnn_a": dict(seed=21, blocks=((16, 5, 1), ("dw", 1, 3, 1, 1), ("pw", 24, 1), ("dw", 1, 5, 7, 0), ("pw", 8, 3), (8, 3, 7)), n_labels=5),
    # un-pooled CONV_2D blocks of every row width: 13 -> 16-byte rows with an even tap count and two 32-row tiles, 24 -> 32-byte
    # rows but 40 outputs (stays on v_dot4), 40 -> 64-byte rows; then a pooled tail
    "mfma_mix": dict(seed=23, ncep=13, blocks=((24, 4, 1), (40, 2, 1), (32, 3, 1), (8, 3, 7)), n_labels=4),
    # one 32-row tile with 64-byte rows (40 channels after a pooled block), then an even-tap pooled tail
    "mfma_mix2": dict(seed=24, ncep=13, blocks=((40, 3, 7), (16, 3, 1), (8, 2, 7)), n_labels=3),
    # the shape of Edge Impulse's default 1-D conv export: Conv(8, k3) - MaxPool(2) - Conv(16, k3) - MaxPool(2) - Dense over
    # 12 x 16 = 192 inputs (a FULLY_CONNECTED input far longer than the shipped models' 10)
    "ei_default": dict(seed=30, ncep=13, blocks=((8, 3, -2), (16, 3, -2)), n_labels=4),           # negative pool: VALID (49 -> 24 -> 12)
    "ei_default_same": dict(seed=32, ncep=13, blocks=((8, 3, 2), (16, 3, 2)), n_labels=4),           # SAME pooling, ragged last windows: 49 -> 25 -> 13
    "ei_default40": dict(seed=31, num_filters=40, ncep=40, low=300, high=0, blocks=((16, 3, -2), (32, 3, -2), (32, 3, 1)), n_labels=12),
    "dscnn_b": dict(seed=22, ncep=10, blocks=(("dw", 2, 7, 7, 3), ("pw", 12, 1), ("dw", 1, 3, 7, 1)), n_labels=3),
    # BASELINE config 5 as worded: 49x40 MFCC, deeper depthwise-separable CNN, 10 keywords (+ noise/unknown); synthetic weights
    # (logit_std: calibrated activation ranges and head, tools/synth_model.py calibrate_head -- a model whose softmax is not saturated)
    "cfg5_dscnn": dict(seed=50, num_filters=40, ncep=40, low=300, high=0, n_labels=12, logit_std=3.5,
                       blocks=((32, 5, 1), ("dw", 1, 5, 1, 1), ("pw", 32, 1), ("dw", 1, 5, 7, 1), ("pw", 32, 1), ("dw", 1, 3, 7, 1), ("pw", 12, 0))),
}


def random_graph_spec(seed):
    """A random member of the 1-D conv graph family within the kernels' documented limits (for the fuzz tests): 1-4 blocks of
    CONV_2D / depthwise / pointwise, taps 1-8, channels 4-48, pooling 1 / 2 / 3 / 7 with SAME (positive) or VALID (negative)
    padding, 2-12 labels.  Returns synth_model_blob keyword arguments, or None when the draw leaves the limits."""
    rng = np.random.default_rng(1000 + seed)
    ncep = int(rng.choice([10, 13, 16, 20]))
    w, c = 49, ncep
    blocks = []
    for b in range(int(rng.integers(1, 5))):
        kind = rng.choice(["conv", "conv", "conv", "dw", "pw"]) if b else "conv"
        pool = int(rng.choice([1, 1, 2, -2, 3, -3, 7]))
        if kind == "conv":
            oc = int(rng.choice([4, 8, 12, 16, 24, 30, 32, 40, 48]))
            blocks.append((oc, int(rng.integers(1, 9)), pool))
            c = oc
        elif kind == "dw":
            mult = int(rng.choice([1, 1, 2]))
            if c * mult > 64:
                return None
            blocks.append(("dw", mult, int(rng.choice([3, 5, 7])), pool, int(rng.choice([0, 1, 3]))))
            c = c * mult
        else:
            oc = int(rng.choice([8, 12, 16, 32]))
            blocks.append(("pw", oc, int(rng.choice([0, 1]))))
            c = oc
            pool = 1
        if pool not in (0, 1):
            p = abs(pool)
            w = w // p if pool < 0 else (w + p - 1) // p
        if w < 1:
            return None
    n_labels = int(rng.integers(2, 13))
    if w * c > 1024 or w * c * n_labels * 4 > 32768:
        return None
    return dict(seed=500 + seed, ncep=ncep, blocks=tuple(blocks), n_labels=n_labels, conv_bias=bool(rng.integers(0, 2)))


def random_dsp_spec(seed):
    """A random MFCC configuration the GPU kernel is built for (fft 256, 32 or 40 filters, 49 frames): cepstra, CMVN window and
    the filterbank's frequency range vary.  Returns (MfccConfig keyword overrides, synth_model_blob keyword arguments)."""
    rng = np.random.default_rng(7000 + seed)
    nf = int(rng.choice([32, 40]))
    ncep = int(rng.integers(2, nf + 1))
    win = int(rng.choice([17, 21, 33, 51, 75, 101, 121, 137])) if ncep > 16 and nf == 40 else int(rng.choice([13, 15, 33, 51, 101, 137]))
    low = int(rng.choice([0, 50, 300, 600]))
    high = int(rng.choice([0, 3500, 4000, 6000]))
    cfg_kw = dict(num_filters=nf, num_cepstral=ncep, win_size=win, low_frequency=low, high_frequency=high)
    blob_kw = dict(seed=900 + seed, num_filters=nf, ncep=ncep, win_size=win, low=low, high=high, blocks=((8, 3, 7), (4, 3, 7)), n_labels=3)
    return cfg_kw, blob_kw


# ---------------------------------------------------------------------------------------------------------------
#  the int8 network at the edges of its quantisation (tests/test_gpu_quant_edges.py, the CPU pins in
#  tests/test_oracle_vs_reference.py, tests/golden/quant_edges_l476.npz)
# ---------------------------------------------------------------------------------------------------------------
# The smallest graphs at which each int8 kernel path still exists (none had to be adjusted: the plan accepts all three).
QUANT_EDGE_GRAPHS = {
    # two-block matrix-core kernel with 16-byte rows; under kws_dev_force_scalar_nn(1) the generic kernel's pooled sdot4 path
    "g2": dict(seed=81, ncep=13, blocks=((24, 3, 7), (8, 3, 7)), n_labels=4),
    # the same blocks behind 40 cepstra: kws_nn_mfma_kernel<64>
    "g2w": dict(seed=82, num_filters=40, ncep=40, low=300, high=0, blocks=((24, 3, 7), (8, 3, 7)), n_labels=4),
    # generic kernel: two un-pooled matrix-core blocks (conv 8, pointwise 12), the four-channel-group depthwise path (multiplier 1)
    # and the general one (multiplier 2), a VALID-pooled sdot4 block with 32-byte rows
    "gd": dict(seed=94, ncep=13, blocks=((8, 3, 1), ("dw", 1, 3, 7, 1), ("pw", 12, 1), ("dw", 2, 3, 1, 0), (4, 3, -2)), n_labels=4),
}
QUANT_EDGE_REQUANT_OPS = {"g2": 2, "g2w": 1, "gd": 5}     # CONV_2D / DEPTHWISE_CONV_2D positions edited per graph (g2w: its first block)
QUANT_EDGE_SPARSE_SEED = 20240611                          # the sparse weights' own generator: nothing is drawn from the model's


class GraphEdit:
    """A synthetic graph's (tensors, nodes) with the operations the edge table needs.  Every setter keeps the graph
    self-consistent: an activation's scale / zero point is changed on every non-constant tensor that shares it (through
    RESHAPE and MAX_POOL_2D, in both directions), and finish() recomputes every int32 bias scale."""

    def __init__(self, tensors, nodes):
        self.t, self.n = tensors, nodes

    def requant(self, k):
        return [nd for nd in self.n if nd["op"] in (1, 6)][k]

    def op(self, code):
        return [nd for nd in self.n if nd["op"] == code][0]

    def group(self, tid):
        g, grew = {tid}, True
        while grew:
            grew = False
            for nd in self.n:
                if nd["op"] in (0, 3) and ((nd["in"][0] in g) != (nd["out"][0] in g)):
                    g |= {nd["in"][0], nd["out"][0]}
                    grew = True
        return g

    def producer(self, tid):
        g = self.group(tid)
        return next((nd for nd in self.n if nd["op"] not in (0, 3) and nd["out"][0] in g), None)

    def consumer(self, tid):
        g = self.group(tid)
        return next((nd for nd in self.n if nd["op"] not in (0, 3) and any(i in g for i in nd["in"])), None)

    def add_behind(self, nd):
        c = self.consumer(nd["out"][0])
        return c if c is not None and c["op"] == 2 else None

    def set_quant(self, tid, scale=None, zero=None):
        for i in self.group(tid):
            if scale is not None:
                self.t[i]["scale"] = [float(np.float32(scale))]
            if zero is not None:
                self.t[i]["zero"] = [int(zero)]

    def drop_activation_of(self, tid):
        """the producer of activation tid loses its fused ReLU (a zero point of +127 under a ReLU leaves one value)"""
        nd = self.producer(tid)
        if nd is not None and nd["op"] in (1, 6):
            nd["p"][3] = 0
        elif nd is not None and nd["op"] in (2, 4):
            nd["p"][0] = 0

    def scale_weights(self, nd, factor):
        tw = self.t[nd["in"][1]]
        tw["scale"] = [float(np.float32(s * factor)) for s in tw["scale"]]

    def set_scales(self, nd, in_scale=None, w_scale=None, out_scale=None, per_tensor=False):
        """scales of a CONV_2D / DEPTHWISE_CONV_2D / FULLY_CONNECTED node.  A new output scale is followed downstream so that
        the ops behind keep the multipliers they were drawn with: an ADD behind has its constant and its output rescaled by the
        same ratio, and the next convolution's / FULLY_CONNECTED's weight scales are divided by it."""
        if in_scale is not None:
            self.set_quant(nd["in"][0], scale=in_scale)
        tw = self.t[nd["in"][1]]
        if w_scale is not None:
            tw["scale"] = [float(np.float32(w_scale))] * len(tw["scale"])
        if per_tensor:
            tw["scale"], tw["zero"] = tw["scale"][:1], tw["zero"][:1]
        if out_scale is not None:
            o = nd["out"][0]
            r = float(np.float32(out_scale)) / self.t[o]["scale"][0]
            self.set_quant(o, scale=out_scale)
            nxt = self.consumer(o)
            if nxt is not None and nxt["op"] == 2:
                tc = self.t[[i for i in nxt["in"] if self.t[i]["const"]][0]]
                tc["scale"] = [float(np.float32(tc["scale"][0] * r))]
                o = nxt["out"][0]
                self.set_quant(o, scale=self.t[o]["scale"][0] * r)
                nxt = self.consumer(o)
            if nxt is not None and nxt["op"] in (1, 4, 6):
                self.scale_weights(nxt, 1.0 / r)

    def set_multiplier(self, nd, eff):
        """weight scales alone (every channel the same) so that in * w / out is eff to float32 precision: nothing else moves"""
        i, o = self.t[nd["in"][0]]["scale"][0], self.t[nd["out"][0]]["scale"][0]
        self.set_scales(nd, w_scale=eff * o / i)

    def set_multiplier_pow2(self, nd, eff):
        """eff (a power of two) EXACTLY: the output scale becomes the input scale times the nearest power of two, the weight
        scales the power of two that is left"""
        i, o = self.t[nd["in"][0]]["scale"][0], self.t[nd["out"][0]]["scale"][0]
        k = int(np.round(np.log2(o / i)))
        self.set_scales(nd, w_scale=eff * 2.0 ** k, out_scale=float(np.float32(i)) * 2.0 ** k)
        ii, oo, ww = (np.float64(self.t[x]["scale"][0]) for x in (nd["in"][0], nd["out"][0], nd["in"][1]))
        assert ii * ww / oo == eff

    def set_bias(self, nd, values):
        tb = self.t[nd["in"][2]]
        n = tb["dims"][0]
        tb["data"] = np.resize(np.asarray(values, np.int64), n).astype(np.int32).tobytes()

    def sparse_weights(self, nd):
        """two +-1 entries per output channel and biases in +-20: a left-shifting op with drawn weights clamps 99 % of its outputs"""
        rng = np.random.default_rng(QUANT_EDGE_SPARSE_SEED)
        tw = self.t[nd["in"][1]]
        dims = tw["dims"]
        if nd["op"] == 6:                                  # [1][1][taps][out_c]: a channel's weights are its taps
            n_out, per = dims[3], dims[2]
            w = np.zeros((per, n_out), np.int8)
            for c in range(n_out):
                w[rng.choice(per, 2, replace=False), c] = rng.choice([-1, 1], 2)
        else:                                              # [out_c][1][taps][in_c] or FULLY_CONNECTED [out][in]
            n_out, per = dims[0], int(np.prod(dims[1:]))
            w = np.zeros((n_out, per), np.int8)
            for c in range(n_out):
                w[c, rng.choice(per, 2, replace=False)] = rng.choice([-1, 1], 2)
        tw["data"] = w.tobytes()
        self.set_bias(nd, rng.integers(-20, 21, n_out))

    def finish(self):
        """every int32 bias scale = float32(input scale) * float32(weight scale[ch]) (kernel_util_lite.cc:47-120 checks that product)"""
        for nd in self.n:
            if nd["op"] in (1, 4, 6) and len(nd["in"]) > 2:
                tw, tb = self.t[nd["in"][1]], self.t[nd["in"][2]]
                i = np.float32(self.t[nd["in"][0]]["scale"][0])
                tb["scale"] = [float(i * np.float32(s)) for s in tw["scale"]]
                tb["zero"] = [0] * len(tw["scale"])


# The triple whose double-precision quotient 0x1.fffffffec003dp-1 rounds to 2^31 in QuantizeMultiplier: multiplier 2^30, shift +1
ROLLOVER_SCALES = (0.05988423526287079, 0.005621093790978193, 0.000336614903062582)
_EFF_M31 = 1.5 * 2.0 ** -32          # frexp: 0.75 * 2^-31 -> shift -31 exactly
_EFF_ZERO = 1.5 * 2.0 ** -33         # frexp: 0.75 * 2^-32 -> shift < -31 -> multiplier 0
# round(x * 0.75 / 2^31) changes at |x| = 2^30 / 0.75: with these biases (sign alternating by channel) the accumulators straddle
# the only rounding boundary a shift of -31 has inside the int32 range, so the output takes zero point - 1, zero point, zero point + 1
_BIAS_M31 = (1431655765, -1431655765)


def _rq_mult_one(g, nd): g.set_multiplier_pow2(nd, 1.0)
def _rq_mult_half(g, nd): g.set_multiplier_pow2(nd, 0.5)
def _rq_mult_1_37(g, nd): g.set_multiplier(nd, 1.37)
def _rq_mult_3(g, nd): g.set_multiplier(nd, 2.9)
def _rq_rollover(g, nd): g.set_scales(nd, *ROLLOVER_SCALES)
def _rq_zero_mult(g, nd): g.set_multiplier(nd, _EFF_ZERO)
def _rq_per_tensor(g, nd): g.set_scales(nd, per_tensor=True)


def _rq_shift_m31(g, nd):
    g.set_multiplier(nd, _EFF_M31)
    g.set_bias(nd, _BIAS_M31)


def _zp(which, value):
    def f(g, nd):
        tid = nd["in"][0] if which == "in" else nd["out"][0]
        if value == 127:
            g.drop_activation_of(tid)
        g.set_quant(tid, zero=value)
    return f


# case -> (edit of one requantising node, its left shift is positive)
QUANT_EDGE_REQUANT_CASES = {
    "mult_one": (_rq_mult_one, True), "mult_half": (_rq_mult_half, False), "mult_1_37": (_rq_mult_1_37, True),
    "mult_3": (_rq_mult_3, True), "rollover": (_rq_rollover, True), "shift_m31": (_rq_shift_m31, False),
    "zero_mult": (_rq_zero_mult, False), "per_tensor": (_rq_per_tensor, False),
    "in_zp_m128": (_zp("in", -128), False), "in_zp_p127": (_zp("in", 127), False),
    "out_zp_m128": (_zp("out", -128), False), "out_zp_p127": (_zp("out", 127), False),
}
# mult_half has shift 0, not a left shift, but its drawn weights clamp as much (measured 0.99): it gets the sparse variant too
QUANT_EDGE_SPARSE_CASES = ("mult_one", "mult_half", "mult_1_37", "mult_3", "rollover")


def _add_const_first(g, ad): ad["in"].reverse()
def _add_act_none(g, ad): ad["p"][0] = 0
def _add_relu6(g, ad): ad["p"][0] = 3
def _add_out_zp(g, ad): g.set_quant(ad["out"][0], zero=-77)


def _add_const_x100(g, ad):
    tc = g.t[[i for i in ad["in"] if g.t[i]["const"]][0]]
    tx = g.t[[i for i in ad["in"] if not g.t[i]["const"]][0]]
    tc["scale"] = [float(np.float32(100.0 * tx["scale"][0]))]
    # one step of the constant is now 100 steps of the other input: the drawn values (-127 .. 0) would push every sum under the ReLU
    tc["data"] = np.random.default_rng(QUANT_EDGE_SPARSE_SEED).integers(-1, 2, tc["dims"][0]).astype(np.int8).tobytes()


QUANT_EDGE_ADD_CASES = {"const_first": _add_const_first, "act_none": _add_act_none, "relu6": _add_relu6, "const_x100": _add_const_x100,
                        "out_zp_m77": _add_out_zp}


def _fc_w_zp(v):
    def f(g): g.t[g.op(4)["in"][1]]["zero"] = [v]
    return f


def _fc_relu(g): g.op(4)["p"][0] = 1
def _fc_out_scale(v):
    def f(g): g.set_quant(g.op(4)["out"][0], scale=v)
    return f


def _beta(v):
    def f(g): g.op(5)["beta"] = v
    return f


QUANT_EDGE_HEAD_CASES = {"fc_w_zp_m7": _fc_w_zp(-7), "fc_w_zp_p9": _fc_w_zp(9), "fc_relu": _fc_relu, "fc_out_scale_2": _fc_out_scale(2.0),
                         "fc_out_scale_1e-4": _fc_out_scale(1e-4), "beta_0.25": _beta(0.25), "beta_4": _beta(4.0)}
QUANT_EDGE_LABELS = (13, 16, 17, 32, 33, 47, 48)          # gd: fc_in = 24 * 4 = 96, 96 * 48 <= 32768


def _wrap(g, nd):
    """requantise-then-max != max-then-requantise: multiplier 1610612881, shift +2, and biases that put (acc + bias) << 2 past 2^31"""
    i = g.t[nd["in"][0]]["scale"][0]
    g.set_scales(nd, w_scale=0.004, out_scale=float(np.float32(i)) * float(np.float32(0.004)) / 3.0)
    g.set_bias(nd, [2 ** 29 - 20000])


def _quant_edges():
    """key -> dict(graph, kw, edit, where): where = ("rq", k) | ("fc",) names the op whose output the non-vacuity conditions look at"""
    out = {}

    def put(key, graph, where, fn, **kw):
        def edit(tensors, nodes):
            g = GraphEdit(tensors, nodes)
            fn(g)
            g.finish()
        out[key] = dict(graph=graph, kw=dict(QUANT_EDGE_GRAPHS[graph], **kw), edit=edit, where=where)

    for graph, n_rq in QUANT_EDGE_REQUANT_OPS.items():
        targets = [("c%d" % k, ("rq", k)) for k in range(n_rq)] + ([("fc", ("fc",))] if graph != "g2w" else [])
        for tname, where in targets:
            def node_of(g, where=where):
                return g.requant(where[1]) if where[0] == "rq" else g.op(4)
            for case, (fn, _) in QUANT_EDGE_REQUANT_CASES.items():
                if where[0] == "fc" and case == "per_tensor":
                    continue                                                   # the FULLY_CONNECTED scale is per tensor already
                put("%s/%s/%s" % (graph, tname, case), graph, where, lambda g, fn=fn, node_of=node_of: fn(g, node_of(g)))
                if case in QUANT_EDGE_SPARSE_CASES:
                    def both(g, fn=fn, node_of=node_of):
                        fn(g, node_of(g))
                        g.sparse_weights(node_of(g))
                    put("%s/%s/%s+sparse" % (graph, tname, case), graph, where, both)
    for graph in ("g2", "gd"):
        n_rq = QUANT_EDGE_REQUANT_OPS[graph]
        adds = [k for k in range(n_rq) if not isinstance(QUANT_EDGE_GRAPHS[graph]["blocks"][k][0], str)]      # (out_c, taps, pool) blocks
        for k in adds:
            for case, fn in QUANT_EDGE_ADD_CASES.items():
                put("%s/add%d/%s" % (graph, k, case), graph, ("add", k), lambda g, fn=fn, k=k: fn(g, g.add_behind(g.requant(k))))
        for case, fn in QUANT_EDGE_HEAD_CASES.items():
            put("%s/head/%s" % (graph, case), graph, ("fc",), fn)
        for n in QUANT_EDGE_LABELS:
            put("%s/labels/%d" % (graph, n), graph, ("fc",), lambda g: None, n_labels=n)
    return out


QUANT_EDGES = _quant_edges()


def _quant_refusals():
    """models kws_create must refuse with KWS_ERROR_UNSUPPORTED_MODEL: key -> synth_model_blob keyword arguments (edit included)"""
    out = {}

    def put(key, kw, k):
        def edit(tensors, nodes):
            g = GraphEdit(tensors, nodes)
            _wrap(g, g.requant(k))
            g.finish()
        out[key] = dict(kw, edit=edit)
    put("wrap/conv8", dict(seed=84, blocks=((8, 3, 7), (4, 3, 7)), add_bias=False), 0)       # the model of the report: 53 of 56 pooled outputs differ
    put("wrap/g2_block2", QUANT_EDGE_GRAPHS["g2"], 1)
    put("wrap/gd_depthwise", QUANT_EDGE_GRAPHS["gd"], 1)
    put("wrap/gd_pointwise", QUANT_EDGE_GRAPHS["gd"], 2)
    out["labels/49"] = dict(QUANT_EDGE_GRAPHS["g2"], n_labels=49)
    return out


QUANT_REFUSALS = _quant_refusals()


def quant_edge_groups():
    """the edge models by graph and edited op ("g2/c0", "gd/add4", "g2/labels", ...): one test case each, the cases of the op inside"""
    return sorted({k.rsplit("/", 1)[0] for k in QUANT_EDGES})


def quant_edge_blob(key):
    e = QUANT_EDGES[key]
    return synth_model_blob(edit=e["edit"], **e["kw"])


def quant_edge_inputs(n_features, golden_rows=False):
    """the input set of test_nn_bit_exact_random_int8 cut to 64 uniform rows, 64 normal(-11, 25) rows and the 256 constant rows;
    golden_rows: the 24 of them tests/golden/quant_edges_l476.npz holds results for (8 uniform, 8 normal, every 32nd constant)"""
    rng = np.random.default_rng(4)
    qs = np.concatenate([rng.integers(-128, 128, (64, n_features)).astype(np.int8),
                         np.clip(rng.normal(-11, 25, (64, n_features)), -128, 127).astype(np.int8),
                         np.repeat(np.arange(-128, 128, dtype=np.int8)[:, None], n_features, 1)])
    return qs[quant_edge_golden_rows()] if golden_rows else qs


def quant_edge_golden_rows():
    return np.concatenate([np.arange(8), 64 + np.arange(8), 128 + np.arange(0, 256, 32)])


def quant_edge_tensor_ids(blob, where):
    """(tensor id of the edited op's output, ids of every block's pooled tensor in block order, FULLY_CONNECTED output id) of a blob"""
    import eon_import
    tensors, nodes, _, _, _ = eon_import.parse_blob(blob)
    g = GraphEdit(tensors, nodes)
    rq = [nd for nd in nodes if nd["op"] in (1, 6)]
    pooled = []
    for k, nd in enumerate(rq):                              # the last activation before the next conv / the FULLY_CONNECTED, minus reshapes
        end = rq[k + 1] if k + 1 < len(rq) else g.op(4)
        tid = end["in"][0]
        while True:
            p = next(n_ for n_ in nodes if n_["out"][0] == tid)
            if p["op"] != 0:
                break
            tid = p["in"][0]
        pooled.append(tid)
    fc = g.op(4)["out"][0]
    if where[0] == "rq":
        edited = rq[where[1]]["out"][0]
    elif where[0] == "add":
        edited = g.add_behind(rq[where[1]])["out"][0]
    else:
        edited = fc
    return edited, pooled, fc


def quant_edge_not_vacuous(key, edited, fc_rows):
    """The conditions that keep a case from testing nothing, on the checker's output of the edited tensor alone (edited: that
    tensor over all input rows; fc_rows: the FULLY_CONNECTED output [rows][labels]).  Returns None or what is wrong.
      * at most 75 % of the values at -128 / 127 and at least 32 distinct values;
      * FULLY_CONNECTED / head / label cases: the FC outputs take at least 5 distinct values;
      * zero_mult: exempt, constant by design;
      * shift_m31: a multiplier below 2^-31 maps the whole int32 range onto at most 3 values, so 32 cannot be asked: the biases
        of _BIAS_M31 put the accumulators on both sides of a rounding boundary, and at least 2 distinct values are required;
      * the drawn-weight variants of the left-shift cases clamp nearly everything (0.99 measured at multipliers 1 and 1/2): the
        conditions are asserted on their +sparse variants, the drawn-weight ones only run."""
    case = key.split("/")[2]
    where = QUANT_EDGES[key]["where"]
    if case == "zero_mult" or case in QUANT_EDGE_SPARSE_CASES:
        return None
    vals = np.unique(fc_rows if where[0] == "fc" else edited)
    if case == "shift_m31":
        return None if len(vals) >= 2 else "%d distinct values" % len(vals)
    if where[0] == "fc":
        return None if len(vals) >= 5 else "FC outputs take %d distinct values" % len(vals)
    share = float(np.isin(edited, (-128, 127)).mean())
    if share > 0.75:
        return "%.2f of the values at the limits" % share
    return None if len(vals) >= 32 else "%d distinct values" % len(vals)


def quant_edge_digest(pooled_rows):
    """[rows][pooled bytes] -> uint8 [rows][8]: the first 8 bytes of each row's SHA-256.  The pooled tensors of gd are 2.6 KB a
    row, 221 models of them would be past any golden file's size; equal digests are equal tensors, and where they differ the
    comparison with the checker's tensors (every test that reads these also makes it) says where."""
    import hashlib
    return np.stack([np.frombuffer(hashlib.sha256(np.ascontiguousarray(r).tobytes()).digest()[:8], np.uint8) for r in pooled_rows])


def quant_edge_run(invoke, blob, where, qs):
    """invoke(q) -> (output, every tensor) over the rows of qs: dict(out, fc, pooled = every block's pooled tensor concatenated in
    block order -- the layout of the library's debug tap --, edited = the edited op's output), each [rows][...] int8"""
    edited, pooled, fc = quant_edge_tensor_ids(blob, where)
    r = dict(out=[], fc=[], pooled=[], edited=[])
    for q in qs:
        o, taps = invoke(q)
        r["out"].append(np.array(o, np.int8))
        r["fc"].append(np.array(taps[fc], np.int8))
        r["pooled"].append(np.concatenate([np.asarray(taps[i], np.int8).reshape(-1) for i in pooled]))
        r["edited"].append(np.array(taps[edited], np.int8).reshape(-1))
    return {k: np.stack(v) for k, v in r.items()}


def quant_edge_golden():
    """tests/golden/quant_edges_l476.npz (tools/make_golden.py --only-quant-edges): key -> dict(out, fc [24][labels] int8,
    pooled_sha [24][8] uint8), the reference's own op registrations on quant_edge_inputs(golden_rows=True)"""
    g = np.load(os.path.join(GOLDEN, "quant_edges_l476.npz"))
    n_rows = len(quant_edge_golden_rows())
    offs = np.cumsum([0] + [int(n) * n_rows for n in g["n_labels"]])
    return {str(k): dict(out=g["out"][offs[i]:offs[i + 1]].reshape(n_rows, -1), fc=g["fc"][offs[i]:offs[i + 1]].reshape(n_rows, -1),
                         pooled_sha=g["pooled_sha"][i]) for i, k in enumerate(g["keys"])}


# ---------------------------------------------------------------------------------------------------------------
#  the float32 network kernels over every blocking and at float edges (tests/test_gpu_f32_edges.py, the CPU pins in
#  tests/test_oracle_vs_reference.py, tests/golden/f32_edges_l476.npz)
# ---------------------------------------------------------------------------------------------------------------
F32_FLT_MAX = float(np.finfo(np.float32).max)


def f32_act_range(act):
    """CalculateActivationRange<float> (kernel_util_lite.h:79-97): TfLiteFusedActivation -> (lo, hi)"""
    return {0: (-F32_FLT_MAX, F32_FLT_MAX), 1: (0.0, F32_FLT_MAX), 2: (-1.0, 1.0), 3: (0.0, 6.0)}[act]


def f32_pick_blocking(depthwise, out_w, out_c, pool, pool_stride, pool_w):
    """kws_nn_f32_pick_blocking restated: (tb, ob, mode), mode "direct" (no pooling node) | "fused" (pooled in registers) | "staged".
    A restatement for choosing and describing test shapes only: the GPU test asserts the library's own pick through kws_dev_f32_blocking."""
    can_fuse = pool > 1 and pool == pool_stride and pool in (2, 4, 7, 8)
    best, pick = [1e30, 1e30], [(1, 1), (1, 1)]
    for fused in (0, 1):
        for tb in (1, 2, 4, 7, 8):
            for ob in (1, 2, 4):
                if depthwise and ob != 1:
                    continue
                if fused and (not can_fuse or tb != pool):
                    continue
                n_tb = pool_w if fused else (out_w + tb - 1) // tb
                items = n_tb * ((out_c + ob - 1) // ob)
                cost = ((items + 63) // 64) * (2 * tb * ob + tb + 1)
                if cost < best[fused]:
                    best[fused], pick[fused] = cost, (tb, ob)
    fused = 1 if can_fuse and best[1] <= best[0] else 0
    tb, ob = pick[fused]
    return tb, ob, "fused" if fused else "direct" if pool == 1 else "staged"


def f32_graph_blocks(blob):
    """The conv blocks of a float .kwsm as build_nn_plan_f32 reads them: per block a dict of the shape, the blocking (f32_pick_blocking),
    the nodes (conv_nd, add_nd, pool_nd: node dicts or None) and the head: (blocks, dict(fc_in, fc_out, dense, n_features))."""
    import eon_import
    tensors, nodes, t_in, _, _ = eon_import.parse_blob(blob)
    blocks = []
    for nd in nodes:
        if nd["op"] in (1, 6):
            blocks.append(dict(conv_nd=nd, add_nd=None, pool_nd=None))
        elif nd["op"] == 2:
            blocks[-1]["add_nd"] = nd
        elif nd["op"] == 3:
            blocks[-1]["pool_nd"] = nd
    for b in blocks:
        cv = b["conv_nd"]
        x, w = tensors[cv["in"][0]]["dims"], tensors[cv["in"][1]]["dims"]
        dw = cv["op"] == 6
        in_w, in_c, taps = x[2], x[3], w[2]
        out_c = w[3] if dw else w[0]
        out_w = in_w if cv["p"][0] == 1 else in_w - taps + 1
        pad_left = max(0, (out_w - 1) + taps - in_w) // 2
        pool = stride = 1
        pool_w = out_w
        if b["pool_nd"] is not None:
            p = b["pool_nd"]["p"]
            pool, stride = p[4], p[2]
            pool_w = (out_w + stride - 1) // stride if p[0] == 1 else (out_w - pool) // stride + 1
        tb, ob, mode = f32_pick_blocking(dw, out_w, out_c, pool, stride, pool_w)
        ntb = pool_w if mode == "fused" else (out_w + tb - 1) // tb
        b.update(depthwise=dw, in_w=in_w, in_c=in_c, taps=taps, out_c=out_c, out_w=out_w, pad_left=pad_left, pool=pool, pool_stride=stride,
                 pool_w=pool_w, pool_valid=b["pool_nd"] is not None and b["pool_nd"]["p"][0] == 2, conv_valid=cv["p"][0] == 2,
                 tb=tb, ob=ob, mode=mode, ntb=ntb, rows=max(pad_left + in_w, ntb * tb + taps - 1))
    fcs = [nd for nd in nodes if nd["op"] == 4]
    dense = len(fcs) > 1 or not blocks
    w = tensors[fcs[0]["in"][1]]["dims"]
    head = dict(fc_in=w[1], fc_out=0 if dense else w[0], dense=dense, n_features=tensors[t_in]["dims"][-1], n_dense=len(fcs) if dense else 0)
    return blocks, head


def f32_launch_shape(blob):
    """(waves per workgroup, dynamic LDS bytes) of kws_nn_f32_kernel for a float blob: kws_nn_f32_waves / kws_nn_f32_smem_bytes / nnf_layout
    restated (test shapes only; the GPU test asserts both against kws_dev_f32_blocking)"""
    blocks, head = f32_graph_blocks(blob)
    r4 = lambda v: (v + 3) & ~3
    w_fl = a_fl = b_fl = y_fl = 0
    for i, b in enumerate(blocks):
        w_fl += (b["taps"] if b["depthwise"] else b["taps"] * b["in_c"]) * r4(b["out_c"])
        img = b["rows"] * b["in_c"]
        if i & 1:
            b_fl = max(b_fl, img)
        else:
            a_fl = max(a_fl, img)
        if b["mode"] == "staged":
            y_fl = max(y_fl, b["out_w"] * b["out_c"])
    fc_fl = r4(head["fc_out"] * head["fc_in"] + head["fc_out"])
    vec_fl = r4(max(head["fc_in"], 64)) + 64
    smem = lambda waves: (w_fl + fc_fl + waves * (r4(a_fl) + r4(b_fl) + r4(y_fl) + vec_fl)) * 4
    vec4 = any(not b["depthwise"] and b["tb"] > 1 and b["in_c"] % 4 == 0 for b in blocks)
    waves = next((w for w in range(8 if vec4 else 16, 4, -1) if smem(w) <= 158 * 1024), 4)
    return waves, smem(waves)


def f32_edit_blob(blob, edit):
    """a float blob with edit(tensors, nodes) applied (edit=None: the blob itself)"""
    if edit is None:
        return blob
    import eon_import
    tensors, nodes, t_in, t_out, meta = eon_import.parse_blob(blob)
    edit(tensors, nodes)
    return eon_import.serialise(tensors, nodes, t_in, t_out, meta)


def f32_blob(entry):
    """entry: dict(kw = synth_model_blob keyword arguments, edit = None or edit(tensors, nodes) of the de-quantised graph) -> float .kwsm"""
    from dequantize_model import dequantize
    return f32_edit_blob(dequantize(synth_model_blob(**entry["kw"])), entry.get("edit"))


def _fget(t):
    return np.frombuffer(t["data"], np.float32).copy()


def _fset(t, v):
    v = np.ascontiguousarray(v, np.float32)
    assert v.nbytes == t["nbytes"], (v.nbytes, t["nbytes"])
    t["data"] = v.tobytes()


def _frames(n, ncep, **kw):
    """DSP geometry for n frames of ncep columns (20 ms frames and stride at 16 kHz: 320 (n + 1) samples)"""
    nf = 32 if ncep <= 32 else 40 if ncep <= 40 else 64
    return dict(dict(raw_samples=320 * (n + 1), ncep=ncep, num_filters=nf, high=0, n_labels=3, add_bias=False, conv_bias=True), **kw)


def _f32_blockings():
    """key "conv|dw/tb<T>/ob<O>/<mode>[#note]" -> dict(kw, block, edit, rows = input rows of f32_inputs).  The block under test is block `block` (block 0 wherever nothing is said).
    Shapes: the smallest that an enumeration of kws_nn_f32_pick_blocking over every out_w <= 198, out_c <= 64, pool window 1 .. 8 with SAME or
    VALID padding (and window 3 / stride 2) finds per blocking, or a neighbour that adds a coverage point; taps and input channels are spread so
    that the points a-i of test_f32_blocking_table_covers_the_kernel occur.  The enumeration finds 56 reachable (depthwise, tb, ob, mode)
    combinations -- all 15 conv (tb, ob) and all 5 depthwise tb in every mode, except that tb 1 cannot fuse (a fused lane owns one window of
    tb = pool >= 2 rows); conv (7, 1) direct and staged are reachable from 129 x 3 on.  All 56 have an entry: none had to be left out.
    A SAME pool is loadable only where its left padding is 0 (build_nn_plan_f32): window * windows - rows <= 1.
    Pools: p SAME, -p VALID, (window, stride, VALID?) as synth_model_blob takes them."""
    T = {}
    in_cs, tapss = (3, 4, 5, 8, 2, 6, 7, 12), (3, 1, 2, 7, 9, 4, 16, 5)
    TAIL = (4, 1, -8)                 # a pooled one-tap block that brings a long output under KWS_FC_IN_MAX

    def put(key, frames, ncep, blocks, block=0, rows=64, **kw):
        assert key not in T, key
        T[key] = dict(kw=_frames(frames, ncep, seed=7000 + len(T), blocks=tuple(blocks), **kw), block=block, edit=None, rows=rows)

    def conv(key, w, c, pool=1, tail=False, valid_conv=False, **kw):
        n = len(T)
        in_c, taps = in_cs[n % 8], tapss[(n // 2 + n) % 8]
        put(key, w + (taps - 1 if valid_conv else 0), in_c, [(c, taps, pool)] + ([TAIL] if tail else []),
            conv_valid=(0,) if valid_conv else (), **kw)

    # ---- CONV_2D, one time step per lane (weights streamed as [oc block][step][ob]; 8 steps per batch, J % 8 one by one)
    put("conv/tb1/ob1/direct", 1, 2, [(1, 1, 1)])                                       # J = 2: no full batch
    put("conv/tb1/ob1/staged", 1, 3, [(1, 7, 2)])                                       # J = 21; a SAME window of one row
    put("conv/tb1/ob2/direct", 5, 4, [(13, 2, 1)])                                      # in_c % 4 == 0, even taps, J = 8
    put("conv/tb1/ob2/staged", 5, 3, [(13, 9, 2)], add_bias=True)                       # 9 taps on 5 rows, ragged SAME window, ADD + ReLU
    put("conv/tb1/ob2/staged#valid_pool", 5, 5, [(13, 3, -2)])                          # the VALID pool drops row 4
    put("conv/tb1/ob2/staged#overlap", 5, 2, [(13, 3, (3, 2, True))])                   # window 3, stride 2
    put("conv/tb1/ob2/direct#valid_conv", 7, 3, [(13, 3, 1)], conv_valid=(0,))          # VALID convolution 7 -> 5 rows
    put("conv/tb1/ob4/direct", 3, 13, [(43, 1, 1)])                                     # J = 13
    put("conv/tb1/ob4/staged", 3, 6, [(43, 4, 2)])
    put("conv/tb1/ob2/direct#behind_vec4", 80, 4, [(1, 3, 2), (13, 1, -8), (13, 3, 1)], block=2)   # block 0 has 16-byte rows: the 256-register build
    # ---- CONV_2D, register blocked
    conv("conv/tb2/ob1/direct", 65, 1)
    conv("conv/tb2/ob1/fused", 65, 1, 2)                                                # SAME, ragged last window
    conv("conv/tb2/ob1/staged", 65, 1, (3, 2, True))                                    # window 3, stride 2
    conv("conv/tb2/ob2/direct", 65, 2)
    conv("conv/tb2/ob2/fused", 67, 2, -2)                                               # VALID drops row 66
    conv("conv/tb2/ob2/staged", 65, 2, 3, add_bias=True)                                # SAME, ragged last window; ADD + ReLU
    conv("conv/tb2/ob4/direct", 97, 3)
    conv("conv/tb2/ob4/fused", 97, 3, 2)
    conv("conv/tb2/ob4/staged", 97, 3, -3)
    conv("conv/tb2/ob1/direct#valid_conv", 65, 1, valid_conv=True)
    conv("conv/tb4/ob1/direct", 65, 3)
    conv("conv/tb4/ob1/fused", 65, 3, -4)
    conv("conv/tb4/ob1/staged", 65, 3, 2)
    conv("conv/tb4/ob2/direct", 77, 5)
    conv("conv/tb4/ob2/fused", 67, 5, 4, add_bias=True)                                 # SAME, ragged last window; ADD + ReLU
    conv("conv/tb4/ob2/staged", 77, 5, 2)
    conv("conv/tb4/ob4/direct", 30, 25)
    conv("conv/tb4/ob4/fused", 30, 25, -4)
    conv("conv/tb4/ob4/staged", 30, 25, (3, 2, False))                                  # overlapping SAME windows
    conv("conv/tb7/ob1/direct", 129, 3)
    conv("conv/tb7/ob1/fused", 85, 5, -7)
    conv("conv/tb7/ob1/staged", 129, 3, 2)
    conv("conv/tb7/ob2/direct", 97, 7)
    conv("conv/tb7/ob2/fused", 97, 7, 7)                                                # SAME, ragged last window
    conv("conv/tb7/ob2/staged", 97, 7, 2)
    conv("conv/tb7/ob4/direct", 198, 7, tail=True)
    conv("conv/tb7/ob4/fused", 198, 7, -7)
    conv("conv/tb7/ob4/staged", 198, 7, 2)
    conv("conv/tb8/ob1/direct", 86, 5)
    conv("conv/tb8/ob1/fused", 86, 5, -8)
    conv("conv/tb8/ob1/staged", 86, 5, 2)
    conv("conv/tb8/ob2/direct", 86, 9)
    conv("conv/tb8/ob2/fused", 87, 9, 8)                                                # SAME, ragged last window
    conv("conv/tb8/ob2/staged", 86, 9, 2)
    conv("conv/tb8/ob4/direct", 65, 25, tail=True)
    conv("conv/tb8/ob4/fused", 65, 25, -8)
    conv("conv/tb8/ob4/staged", 65, 25, 2, add_bias=True)
    # ---- DEPTHWISE_CONV_2D ("dw", depth multiplier, taps, pool, activation)
    put("dw/tb1/ob1/direct", 1, 1, [("dw", 1, 3, 1, 0)])
    put("dw/tb1/ob1/staged", 1, 1, [("dw", 1, 1, 2, 0)])
    put("dw/tb2/ob1/direct", 5, 13, [("dw", 1, 3, 1, 0)])
    put("dw/tb2/ob1/fused", 5, 13, [("dw", 1, 5, 2, 0)])                                # SAME, ragged last window
    put("dw/tb2/ob1/staged", 5, 13, [("dw", 1, 7, 3, 0)])                               # SAME, ragged last window
    put("dw/tb2/ob1/staged#overlap", 5, 13, [("dw", 1, 2, (3, 2, True), 0)])
    put("dw/tb2/ob1/direct#valid_conv", 7, 13, [("dw", 1, 3, 1, 0)], conv_valid=(0,))
    put("dw/tb2/ob1/direct#behind_vec4", 80, 4, [(1, 3, 2), (13, 1, -8), ("dw", 1, 3, 1, 0)], block=2)
    put("dw/tb4/ob1/direct", 97, 2, [("dw", 1, 3, 1, 0)])
    put("dw/tb4/ob1/fused", 97, 1, [("dw", 2, 4, -4, 0)])                               # depth multiplier 2; VALID drops row 96
    put("dw/tb4/ob1/staged", 97, 2, [("dw", 1, 16, 2, 0)])
    put("dw/tb7/ob1/direct", 7, 7, [("dw", 7, 3, 1, 0)])
    put("dw/tb7/ob1/fused", 7, 7, [("dw", 7, 5, 7, 1)])                                 # fused ReLU
    put("dw/tb7/ob1/staged", 7, 7, [("dw", 7, 9, 2, 0)])
    put("dw/tb8/ob1/direct", 15, 13, [("dw", 2, 3, 1, 0)])
    # (a window of 8 rows: a row wins one input in 8, and the edge row with two taps fewer -- 160 rows of input bring every position to a win)
    put("dw/tb8/ob1/fused", 11, 5, [("dw", 7, 3, -8, 0)], rows=160)                     # VALID drops rows 8 .. 10
    put("dw/tb8/ob1/fused#ragged", 15, 13, [("dw", 2, 3, 8, 0)])
    put("dw/tb8/ob1/staged", 15, 13, [("dw", 2, 7, 2, 3)])                              # fused ReLU6
    return T


F32_BLOCKINGS = _f32_blockings()


def f32_blocking_name(b):
    """a block of f32_graph_blocks (or the accessor's values in the same keys) -> "conv|dw/tb<T>/ob<O>/<mode>" """
    return "%s/tb%d/ob%d/%s" % ("dw" if b["depthwise"] else "conv", b["tb"], b["ob"], b["mode"])


def f32_inputs(n_features, n=64, seed=476):
    """the feature rows of the blocking tests: n rows of independent N(0, 2^2) values (the network-only entry point takes any vector)"""
    return (np.random.default_rng(seed).standard_normal((n, n_features)) * np.float32(2.0)).astype(np.float32)


F32_GOLDEN_ROWS = 4            # tests/golden/f32_edges_l476.npz holds the reference's logits and scores of the first 4 rows per graph


def f32_reach_shares(blob, invoke, xs):
    """Against a vacuous comparison: per conv block of a float blob, the share of conv output positions (t, oc) that, for at least one row of
    xs, lie strictly inside every clamp range behind them in the block (the convolution's, the ADD's, the pool's fused activation) AND win
    their pooling window -- so that a wrong value there changes the block's output.  Positions no pooling window covers (the tail a VALID pool
    drops) cannot reach any output by the op's definition and are left out of the count.  invoke(x) -> (scores, every tensor)."""
    blocks, _ = f32_graph_blocks(blob)
    reached = [np.zeros((b["out_w"], b["out_c"]), bool) for b in blocks]
    covered = []
    for b in blocks:
        cov = np.zeros(b["out_w"], bool)
        for pw in range(b["pool_w"]):
            cov[pw * b["pool_stride"]:pw * b["pool_stride"] + b["pool"]] = True
        covered.append(cov)
    for x in xs:
        _, taps = invoke(x)
        for b, r in zip(blocks, reached):
            shape = (b["out_w"], b["out_c"])
            v = np.asarray(taps[b["conv_nd"]["out"][0]]).reshape(shape)
            lo, hi = f32_act_range(b["conv_nd"]["p"][3])
            ok = (v > lo) & (v < hi)
            if b["add_nd"] is not None:
                v = np.asarray(taps[b["add_nd"]["out"][0]]).reshape(shape)
                lo, hi = f32_act_range(b["add_nd"]["p"][0])
                ok &= (v > lo) & (v < hi)
            if b["pool_nd"] is not None:
                lo, hi = f32_act_range(b["pool_nd"]["p"][5])
                win = np.zeros(shape, bool)
                for pw in range(b["pool_w"]):
                    rows = slice(pw * b["pool_stride"], min(pw * b["pool_stride"] + b["pool"], b["out_w"]))
                    m = v[rows].max(axis=0)
                    win[rows] |= (v[rows] == m) & (m > lo) & (m < hi)
                ok &= win
            r |= ok
    return [float(r[c].mean()) for r, c in zip(reached, covered)]


def f32_blocking_coverage(blobs):
    """the coverage points a-i of the issue counted from the table: class ("conv_tb>1" | "conv_tb1" | "dw") -> set of point names that occur
    at the block under test of some entry.  blobs: key -> float blob."""
    out = {"conv_tb>1": set(), "conv_tb1": set(), "dw": set()}
    for key, blob in blobs.items():
        b = f32_graph_blocks(blob)[0][F32_BLOCKINGS[key]["block"]]
        pts = out["dw" if b["depthwise"] else "conv_tb1" if b["tb"] == 1 else "conv_tb>1"]
        pts.add("in_c%4==0" if b["in_c"] % 4 == 0 else "in_c%4!=0")
        if b["out_c"] % b["ob"]:
            pts.add("out_c%ob!=0")
        if b["out_c"] % 4:
            pts.add("out_c%4!=0")
        if b["out_w"] % b["tb"]:
            pts.add("out_w%tb!=0")
        t = b["taps"]
        pts.add("taps1" if t == 1 else "taps7" if t == 7 else "taps9..16" if t >= 9 else "taps_even" if t % 2 == 0 else "taps_other")
        if t >= 9 and t % 2 == 0:
            pts.add("taps_even")
        J = t * b["in_c"]
        pts.add("J<8" if J < 8 else "J>8,J%8!=0" if J % 8 else "J%8==0")
        if b["pool"] > 1:
            last = (b["pool_w"] - 1) * b["pool_stride"] + b["pool"]
            if not b["pool_valid"] and last > b["out_w"]:
                pts.add("same_ragged_" + b["mode"])
            if b["pool_valid"] and last < b["out_w"]:
                pts.add("valid_pool_drops_tail")
            if (b["pool"], b["pool_stride"]) == (3, 2):
                pts.add("overlapping_pool")
        if b["conv_valid"]:
            pts.add("valid_conv")
        pts.add("waves<=8" if f32_launch_shape(blob)[0] <= 8 else "waves>8")
    return out


# ---- float edges: activations on every op, subnormals, signed zeros, overflow, softmax, refusals ----
F32_EDGE_GRAPHS = {
    "ca13": dict(seed=8101, ncep=13, blocks=((12, 3, 7), (12, 3, 7)), n_labels=12),                      # conv -> ADD -> pool, twice
    "ca16": dict(seed=8102, ncep=16, blocks=((12, 3, 7), (12, 3, 7)), n_labels=12),                      # ... with 16-byte rows
    "dwpw": dict(seed=8103, ncep=13, blocks=(("dw", 1, 3, 7, 0), ("pw", 12, 0)), n_labels=12),           # depthwise + pointwise pair
    "cd": dict(seed=8104, ncep=13, blocks=((12, 3, 7),), dense=((12, 1),), n_labels=12, add_bias=False),  # trunk kernel + kws_dense_f32_kernel
    "cp13": dict(seed=8105, ncep=13, blocks=((12, 3, 7), (12, 3, 7)), n_labels=4, add_bias=False),       # conv -> pool twice, no additive constant but the head's
    "c1": dict(seed=8106, ncep=13, blocks=((4, 3, 1),), n_labels=4, add_bias=False),                     # one un-pooled conv: a NaN is not dropped by a max
}
# op under test -> (op code, index among the nodes of that code); "head" / "hidden": FULLY_CONNECTED
F32_EDGE_OPS = {
    "ca13": dict(conv0=(1, 0), add0=(2, 0), pool0=(3, 0), conv1=(1, 1), add1=(2, 1), pool1=(3, 1), head=(4, 0)),
    "ca16": dict(conv0=(1, 0), add0=(2, 0), pool0=(3, 0)),
    "dwpw": dict(dw0=(6, 0), pool0=(3, 0), pw1=(1, 0), head=(4, 0)),
    "cd": dict(conv0=(1, 0), pool0=(3, 0), hidden=(4, 0), head=(4, 1)),
}
F32_ACT_NAMES = {0: "none", 1: "relu", 2: "relu_n1_to_1", 3: "relu6"}
_ACT_SLOT = {1: 3, 6: 3, 2: 0, 3: 5, 4: 0}                   # where a node's options hold its TfLiteFusedActivation


def f32_bound_values():
    """-1, 0, 1 and 6 and the float32 values one ulp either side of each: what an additive constant is set to so that a zero input lands a
    pre-activation exactly there"""
    out = []
    for b in (-1.0, 0.0, 1.0, 6.0):
        b = np.float32(b)
        out += [b, np.nextafter(b, np.float32(-np.inf)), np.nextafter(b, np.float32(np.inf))]
    return np.array(out, np.float32)


def _nodes_of(nodes, code):
    return [nd for nd in nodes if nd["op"] == code]


def _additive(tensors, nodes, nd):
    """the tensor of node nd's additive constant (conv / depthwise / FULLY_CONNECTED bias, ADD constant), or None"""
    if nd["op"] == 2:
        return tensors[[i for i in nd["in"] if tensors[i]["const"]][0]]
    if nd["op"] in (1, 4, 6) and len(nd["in"]) > 2 and nd["in"][2] >= 0:
        return tensors[nd["in"][2]]
    return None


def _act_edit(graph, op, act):
    """Small-integer weights (-2 .. 2), every additive constant 0, every activation none -- then the op under test gets activation act and the
    additive constant that feeds it (its own bias / ADD constant; for a pool the constant of the op in front) cycles through
    f32_bound_values(): on an all-zero input every pre-activation of the op IS that constant, exactly."""
    code, idx = F32_EDGE_OPS[graph][op]

    def edit(tensors, nodes):
        rng = np.random.default_rng(F32_EDGE_SEED)
        for nd in nodes:
            if nd["op"] in _ACT_SLOT:
                nd["p"][_ACT_SLOT[nd["op"]]] = 0
            if nd["op"] in (1, 4, 6):
                tw = tensors[nd["in"][1]]
                _fset(tw, rng.integers(-2, 3, tw["nbytes"] // 4))
            ta = _additive(tensors, nodes, nd)
            if ta is not None:
                _fset(ta, np.zeros(ta["nbytes"] // 4))
        target = _nodes_of(nodes, code)[idx]
        target["p"][_ACT_SLOT[code]] = act
        src = target
        if code == 3:                                          # the op in front of the pool that adds a constant
            k = nodes.index(target)
            src = [nd for nd in nodes[:k] if _additive(tensors, nodes, nd) is not None][-1]
        ta = _additive(tensors, nodes, src)
        _fset(ta, np.resize(f32_bound_values(), ta["nbytes"] // 4))
    return edit


F32_EDGE_SEED = 20241019


def _scale(tensors, nd, which, k):
    """multiply a node's weights ("w") or additive constant ("b") by 2^k (exact)"""
    t = tensors[nd["in"][1]] if which == "w" else _additive(tensors, None, nd)
    if t is not None:
        _fset(t, _fget(t) * np.float32(2.0) ** k)


def _subnormal_edit(flushed):
    """block 0's weights x 2^-120 (its additive constant x 2^-132), the next multiplying op's weights x 2^+100, every later additive constant
    x 2^-32 (so that it does not swamp what block 0 hands on).  With inputs of 2^-12 N(0, 2^2) every block-0 activation is subnormal (or zero)
    and the logits are normal.  flushed: the twin whose block 0 produces zeros -- what a flush of its outputs would leave."""
    def edit(tensors, nodes):
        mult = [nd for nd in nodes if nd["op"] in (1, 4, 6)]
        _scale(tensors, mult[0], "w", -120)
        _scale(tensors, mult[0], "b", -132)
        _scale(tensors, mult[1], "w", 100)
        first = nodes.index(mult[0])
        for nd in nodes[first + 1:]:
            if nd["op"] in (1, 2, 4, 6):
                if nd["op"] == 2 and nodes.index(nd) < nodes.index(mult[1]):
                    _scale(tensors, nd, "b", -132)              # block 0's own ADD
                else:
                    _scale(tensors, nd, "b", -32)
        if flushed:
            for nd in nodes[first:nodes.index(mult[1])]:
                for t in ((tensors[nd["in"][1]] if nd["op"] in (1, 6) else None), _additive(tensors, nodes, nd) if nd["op"] in (1, 2, 6) else None):
                    if t is not None:
                        _fset(t, np.zeros(t["nbytes"] // 4))
    return edit


def _zeros_edit(value):
    """every additive constant of the graph := value (+0.0 or -0.0)"""
    def edit(tensors, nodes):
        for nd in nodes:
            ta = _additive(tensors, nodes, nd) if nd["op"] in (1, 2, 4, 6) else None
            if ta is not None:
                _fset(ta, np.full(ta["nbytes"] // 4, value, np.float32))
    return edit


def _overflow_edit(act):
    """block 0's weights become |w| 2^100 and its activation act: with the rows of f32_case_inputs(("signed", 40)) -- finite values of 2^40 N(0, 2^2),
    all positive in rows 0 .. 31, all negative in rows 32 .. 47, mixed behind -- every product overflows: the sums are +inf, -inf, and NaN (inf - inf)"""
    def edit(tensors, nodes):
        cv = [nd for nd in nodes if nd["op"] in (1, 6)][0]
        tw = tensors[cv["in"][1]]
        _fset(tw, np.abs(_fget(tw)))
        _scale(tensors, cv, "w", 100)
        cv["p"][3] = act
    return edit


def _softmax_edit(beta=None, apart=None, equal=False):
    def edit(tensors, nodes):
        if beta is not None:
            _nodes_of(nodes, 5)[0]["beta"] = beta
        fc = _nodes_of(nodes, 4)[-1]
        tb = _additive(tensors, nodes, fc)
        if apart is not None:
            _fset(tb, np.arange(tb["nbytes"] // 4) * np.float32(apart))
        if equal:
            _fset(tensors[fc["in"][1]], np.zeros(tensors[fc["in"][1]]["nbytes"] // 4))
            _fset(tb, np.full(tb["nbytes"] // 4, 1.5, np.float32))
    return edit


def _f32_edges():
    """key "<family>/<graph>/<case>" -> dict(kw, edit, inputs): inputs "edge" (f32_edge_inputs), an exponent k (f32_inputs x 2^k) or ("signed", k)
    (f32_case_inputs)"""
    E = {}

    def put(key, graph, edit, inputs="edge", **kw):
        assert key not in E, key
        E[key] = dict(kw=dict(F32_EDGE_GRAPHS[graph], **kw), edit=edit, inputs=inputs, graph=graph)

    for graph, ops in F32_EDGE_OPS.items():
        for op in ops:
            for act, an in F32_ACT_NAMES.items():
                put("act_%s_%s/%s" % (graph, op, an), graph, _act_edit(graph, op, act))
    for graph in ("cp13", "dwpw"):
        put("subnormal/%s" % graph, graph, _subnormal_edit(False), inputs=-12)
    put("zeros/cp13_bias_free", "cp13", _zeros_edit(0.0))
    put("zeros/cp13_neg_zero_bias", "cp13", _zeros_edit(-0.0))
    put("zeros/ca13_neg_zero_constants", "ca13", _zeros_edit(-0.0))
    put("zeros/dwpw_neg_zero_bias", "dwpw", _zeros_edit(-0.0))
    put("overflow/cp13_relu6", "cp13", _overflow_edit(3), inputs=("signed", 40))
    put("overflow/cp13_none", "cp13", _overflow_edit(0), inputs=("signed", 40))
    put("overflow/c1_none", "c1", _overflow_edit(0), inputs=("signed", 40))              # NaN logits and scores in the mixed rows
    put("softmax/beta_0.25", "cp13", _softmax_edit(beta=0.25))
    put("softmax/beta_4", "cp13", _softmax_edit(beta=4.0))
    put("softmax/logits_200_apart", "cp13", _softmax_edit(apart=200.0))
    put("softmax/logits_equal", "cp13", _softmax_edit(equal=True))
    for n in (2, 47, 48):
        put("softmax/labels_%d" % n, "cp13", None, n_labels=n)
    return E


F32_EDGES = _f32_edges()


def f32_edge_groups():
    return sorted({k.split("/")[0] for k in F32_EDGES})


def f32_edge_inputs(n_features, n=64):
    """row 0 all +0.0, row 1 all -0.0, row 2 alternating +-0.0, rows 3 .. n - 17 small integers (-3 .. 3: with integer weights every sum is
    exact), the last 16 rows N(0, 2^2)"""
    rng = np.random.default_rng(F32_EDGE_SEED + 1)
    x = rng.integers(-3, 4, (n, n_features)).astype(np.float32)
    x[0] = 0.0
    x[1] = -0.0
    x[2] = np.where(np.arange(n_features) % 2, np.float32(-0.0), np.float32(0.0))
    x[n - 16:] = (rng.standard_normal((16, n_features)) * np.float32(2.0)).astype(np.float32)
    return x


def f32_case_inputs(entry, n_features):
    """the input rows of an F32_BLOCKINGS / F32_EDGES entry"""
    if "inputs" not in entry:
        return f32_inputs(n_features, entry["rows"])
    if entry["inputs"] == "edge":
        return f32_edge_inputs(n_features)
    if isinstance(entry["inputs"], tuple):                    # ("signed", k)
        x = (f32_inputs(n_features) * np.float32(2.0) ** entry["inputs"][1]).astype(np.float32)
        x[:32] = np.abs(x[:32])
        x[32:48] = -np.abs(x[32:48])
        return x
    return (f32_inputs(n_features) * np.float32(2.0) ** entry["inputs"]).astype(np.float32)


def f32_all_cases():
    """every table graph, blockings then edges: key -> entry (tools/make_golden.py, the golden and reference pins)"""
    return dict([("blocking/" + k, e) for k, e in F32_BLOCKINGS.items()] + [("edge/" + k, e) for k, e in F32_EDGES.items()])


def _set_weight(code, idx, value, element=5):
    def edit(tensors, nodes):
        tw = tensors[_nodes_of(nodes, code)[idx]["in"][1]]
        w = _fget(tw)
        w[element % w.size] = value
        _fset(tw, w)
    return edit


def _f32_refusals():
    """float graphs kws_create must refuse with KWS_ERROR_UNSUPPORTED_MODEL: key -> dict(kw, edit, says = a piece of kws_last_error's text)"""
    g = F32_EDGE_GRAPHS
    R = {
        "labels_49": dict(kw=dict(g["cp13"], n_labels=49), edit=None, says="FULLY_CONNECTED"),
        "taps_17": dict(kw=dict(g["cp13"], blocks=((12, 17, 7), (12, 3, 7))), edit=None, says="conv"),
        "out_channels_65": dict(kw=dict(g["cp13"], blocks=((65, 3, 7), (12, 3, 7))), edit=None, says="conv"),
        "pool_window_9": dict(kw=dict(g["cp13"], blocks=((12, 3, (9, 9, True)), (12, 3, 1))), edit=None, says="pool"),
        "nine_conv_blocks": dict(kw=dict(g["cp13"], blocks=((8, 3, 1),) + (("pw", 8, 0),) * 8), edit=None, says="conv blocks"),
        "weights_past_lds": dict(kw=dict(g["cp13"], blocks=((64, 16, 1), (64, 16, 7)), n_labels=2), edit=None, says="LDS"),
    }
    inf, nan = np.float32(np.inf), np.float32(np.nan)
    for key, graph, code, idx, v in (("conv0_inf", "cp13", 1, 0, inf), ("conv1_neg_inf", "cp13", 1, 1, -inf), ("conv0_nan", "ca16", 1, 0, nan),
                                     ("depthwise_nan", "dwpw", 6, 0, nan), ("pointwise_inf", "dwpw", 1, 0, inf), ("head_inf", "cp13", 4, 0, inf),
                                     ("head_nan", "ca13", 4, 0, nan), ("hidden_nan", "cd", 4, 0, nan), ("dense_head_neg_inf", "cd", 4, 1, -inf)):
        R["non_finite/" + key] = dict(kw=dict(g[graph]), edit=_set_weight(code, idx, v), says="non-finite")
    return R


F32_REFUSALS = _f32_refusals()

# graphs whose waves serve a second and later clip in a batch of 2 x resident + 37 (tests/test_gpu_f32_edges.py): key -> (kw, what the plan must show)
F32_MULTIPASS = {
    "b512_prefetch": (dict(seed=8201, ncep=16, blocks=((30, 7, 7), (10, 7, 7))), dict(waves_max=8, prefetch=True)),
    "b512_no_prefetch": (dict(seed=8202, ncep=13, blocks=((8, 3, 1), (9, 3, 7))), dict(waves_max=8, prefetch=False)),
    "b1024": (dict(seed=8203, ncep=13, blocks=((30, 7, 7), (10, 7, 7))), dict(waves_min=9, prefetch=False)),
    "dense": (dict(seed=8204, ncep=16, blocks=((30, 7, 7),), dense=((16, 1),), n_labels=4), dict(waves_max=8, prefetch=False)),
}


def f32_prefetch_eligible(blob):
    """pf_ok of kws_nn_f32_generic.h: the first block's padded image and the feature vector are 16-byte aligned, and there is a second block"""
    blocks, head = f32_graph_blocks(blob)
    k = blocks[0]
    lo = k["pad_left"] * k["in_c"]
    hi = lo + k["in_w"] * k["in_c"]
    return (lo | hi | head["n_features"]) & 3 == 0 and (k["rows"] * k["in_c"] + 3) // 4 <= 64 * 9 and len(blocks) > 1


def f32_golden():
    """tests/golden/f32_edges_l476.npz (tools/make_golden.py --only-f32-edges): f32_all_cases key -> dict(logits, scores [F32_GOLDEN_ROWS][labels]),
    the reference's own float op registrations on the first F32_GOLDEN_ROWS input rows of the case"""
    g = np.load(os.path.join(GOLDEN, "f32_edges_l476.npz"))
    offs = np.cumsum([0] + [int(n) * F32_GOLDEN_ROWS for n in g["n_labels"]])
    return {str(k): dict(logits=g["logits"][offs[i]:offs[i + 1]].reshape(F32_GOLDEN_ROWS, -1),
                         scores=g["scores"][offs[i]:offs[i + 1]].reshape(F32_GOLDEN_ROWS, -1)) for i, k in enumerate(g["keys"])}


def same_bits_or_both_nan(a, b):
    a = np.asarray(a, np.float32)
    b = np.asarray(b, np.float32)
    return a.shape == b.shape and bool(((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())
