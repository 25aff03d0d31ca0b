"""Helpers of the recording-scan tests (kws_scan_recordings_device): the restated run_classifier_continuous() fed one recording slice by
slice, with the end-of-signal sample the contract in include/kws/kws.h defines, and the test recordings."""
import ctypes as C

import numpy as np

SLICE = 4000


def wrap_sample(rec, k, slice_samples, grow):
    """what get_data(total_length - 1, 1) of slice k delivers: the recording's sample there, converted like every other sample, or 0
    where the read falls past the recording's end.  Slice 0 claims only itself (its own last sample); every later slice has grown by
    one frame length"""
    p = k * slice_samples + slice_samples + (grow if k > 0 else 0) - 1
    return np.float32(rec[p]) * np.float32(1.0 / 32768.0) if p < rec.size else np.float32(0.0)


def oracle_scan(om, rec, slice_samples=SLICE):
    """scores [W][labels] of one recording through a fresh kwso_continuous (oracle/kws_oracle.c), window after window"""
    L = om.o.L
    grow = int(np.float32(om.cfg.frame_length) * np.float32(om.cfg.sampling_frequency))
    h = L.kwso_continuous_create(om.h)
    assert h
    out = []
    try:
        s = np.zeros(om.n_labels, np.float32)
        produced = C.c_int()
        eos = np.zeros(1, np.float32)
        for k in range(rec.size // slice_samples):
            sl = np.ascontiguousarray(rec[k * slice_samples:(k + 1) * slice_samples], np.int16)
            eos[0] = wrap_sample(rec, k, slice_samples, grow)
            rc = L.kwso_continuous_step(h, sl.ctypes.data, sl.size, eos.ctypes.data, s.ctypes.data, C.byref(produced))
            assert rc == 0, rc
            if produced.value:
                out.append(s.copy())
    finally:
        L.kwso_continuous_free(h)
    return np.array(out, np.float32).reshape(-1, om.n_labels)


def moving_average(raw, taps=2):
    """run_moving_average_filter (ei_run_classifier.h:134-145) over [W][labels], fresh filters, in float32 operation by operation"""
    raw = np.asarray(raw, np.float32)
    out = np.empty_like(raw)
    rs = np.zeros(raw.shape[1], np.float32)
    buf = np.zeros((taps, raw.shape[1]), np.float32)
    for w in range(raw.shape[0]):
        i = w % taps
        rs = (rs - buf[i]).astype(np.float32)
        rs = (rs + raw[w]).astype(np.float32)
        buf[i] = raw[w]
        out[w] = (rs / np.float32(taps)).astype(np.float32)
    return out


def speech(oracle, seed, n):
    """n samples of the synthetic speech-like clips, end to end"""
    k = (n + 15999) // 16000
    return np.ascontiguousarray(oracle.synth(seed, 0, max(k, 1)).reshape(-1)[:n], np.int16)


def pack(recs, seed=0, max_gap=37):
    """recordings packed into one int16 buffer at odd sample offsets, the gaps filled with loud noise (a read outside a recording shows)"""
    rng = np.random.default_rng(seed)
    parts, offs, pos = [], [], 0
    for r in recs:
        gap = int(rng.integers(1, max_gap)) | 1
        parts.append(rng.integers(-30000, 30000, gap).astype(np.int16))
        pos += gap
        offs.append(pos)
        parts.append(np.asarray(r, np.int16))
        pos += r.size
    parts.append(rng.integers(-30000, 30000, 64).astype(np.int16))
    return np.concatenate(parts), np.array(offs, np.uint64), np.array([r.size for r in recs], np.uint64)


def recordings(oracle, seed=1):
    """about 40 recordings: empty, shorter than a window, exactly 4 slices, 4 slices + 1 sample, the last wrap sample just outside /
    just inside, 60 s; speech-like audio, digital silence, DC, audio that goes silent mid-recording"""
    g = 320                                                        # the shipped models' frame length in samples
    lengths = [0, 1, 3999, 4000, 15999, 16000, 16001, 16000 + g - 1, 16000 + g, 20000 + g - 1, 20000 + g, 23999, 24000, 960000]
    recs = []
    for i, n in enumerate(lengths):
        recs.append(speech(oracle, seed * 100 + i, n))
    rng = np.random.default_rng(seed)
    for i in range(14):
        recs.append(speech(oracle, seed * 100 + 20 + i, int(rng.integers(16000, 80000))))
    recs.append(np.zeros(40000, np.int16))                         # digital silence
    recs.append(np.full(36000 + g, 1234, np.int16))                # DC
    recs.append(np.full(28000, -700, np.int16))
    for i in range(4):                                             # goes silent mid-recording
        r = speech(oracle, seed * 100 + 40 + i, 48000 + 4000 * i + 17 * i)
        r[20000 + 1111 * i:] = 0
        recs.append(r)
    recs.append(speech(oracle, seed * 100 + 50, 960000))           # a second 60 s recording
    for i in range(3):
        recs.append(speech(oracle, seed * 100 + 60 + i, 16000 + 4000 * i + g - 1 + (i & 1)))
    return recs
