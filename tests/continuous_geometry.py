"""The geometry grid of the continuous-mode tests (tests/test_continuous_geometry.py without a GPU, tests/test_gpu_continuous_geometry.py
with one): models at frame geometries other than the shipped one, the slicings each accepts and the ones the library refuses, a restatement
of the reference's slice walk, and the layout classes the grid must keep covering.

The slice walk (ei_run_classifier.h:184-282, with the growth of ei_run_dsp.h:319-325): slice 0 claims its own samples, every later slice
`grow = (size_t)(frame_length * frequency)` more; a slice of n_claimed samples gives nf = floor((n_claimed - frame) / stride) frames of
`cols` features, written at slice_offset of the F = rows x cols feature buffer; slice_offset moves on until the buffer is full.  From
the step k_full where it is, every step produces a window, and the rolling buffer then holds ring_rows rows (the rows behind it stay 0).
A live stream keeps keep = ring_rows - nf1 rows between slices."""
import ctypes as C
import os

import numpy as np

from kws_testlib import MODELS, ROOT
from scan_testlib import speech

FREQ = 16000
SMALL = dict(blocks=((8, 3, 1), (4, 3, 1)), n_labels=3)
FRAME_BELOW_20MS = float(np.nextafter(np.float32(0.02), np.float32(0)))     # 320 samples by rounding, 319 by truncation

# name -> (source, accepted slicings, refused slicings {slice: (code, rule)}).  source: a shipped file, or synth_model_blob keyword arguments
# (+ "f32": True for the float32 twin of the int8 graph, tools/dequantize_model.py).  Codes: -5 EI_IMPULSE_DSP_ERROR.  The rules are those
# of scan_layout (csrc/kws_scan.cpp), which are kws_streams_step_device's:
#   "align"   a tuned (non-generic) plan reads int16 slices as 16-byte rows: slice_samples must be a multiple of 8;
#   "past"    the last frame of a slice would read past it ((nf - 1) stride + min(fft, frame) > slice): the reference's get_data of that
#             frame fails too -- the oracle refuses the same step;
#   "nf"      fewer than one frame, or more feature rows than the window holds -- the oracle refuses too;
#   "frames"  a tuned plan's kernel holds at most kws_mfcc_max_frames frames per slice;
GRID = {
    "l476": ("l476_no_yes.kwsm", [2000, 3200, 4000, 4160, 8000], {4001: (-5, "align"), 4004: (-5, "align"), 16000: (-5, "nf"), 100: (-5, "nf")}),
    "l476_f32": ("l476_no_yes_f32.kwsm", [2000, 4160, 8000], {1999: (-5, "align")}),
    # stride 30 ms over 20 ms frames: 32 rows, a whole window per slice at 10 000 samples (k_full = keep = 0)
    "stride30": (dict(SMALL, frame_stride=0.03, win_size=31), [3200, 4000, 10000], {4003: (-5, "align"), 16000: (-5, "nf")}),
    # a frame length whose samples round to 320 but whose growth truncates to 319
    "frame_below_20ms": (dict(SMALL, frame_length=FRAME_BELOW_20MS), [4000, 8000, 16000], {16320: (-5, "nf")}),
    # 2 s, 40 filters: 99 rows (general plan, tuned spectral kernel in chunks)
    "two_s_40f": (dict(raw_samples=32000, num_filters=40, ncep=20, blocks=((8, 3, 1), (4, 3, 1)), n_labels=3), [4000, 12000, 6400], {}),
    # a 4000-sample window: 11 rows
    "clip4000": (dict(SMALL, raw_samples=4000), [1000, 2000, 2080], {4000: (-5, "nf")}),
    # 10 ms stride: 98 rows, overlapping frames; odd slices on the general kernels
    "stride10": (dict(SMALL, frame_stride=0.01, win_size=31), [2399, 3999, 6239], {4000: (-5, "past"), 2000: (-5, "past"), 1: (-5, "nf")}),
    # 321-sample frames every 161 into a 512-point FFT: the cooperative general kernel, odd slices
    "odd_stride_fft512": (dict(SMALL, fft_length=512, frame_length=0.0200625, frame_stride=0.0100625, win_size=31), [2575, 3219, 5151], {2577: (-5, "past"), 3220: (-5, "past")}),
    "fft128_win51": (dict(SMALL, fft_length=128, win_size=51), [2000, 3200, 5440], {}),
    # MFE block at a 0.5 s window with 40 filters: 24 rows
    "mfe_500ms": (dict(SMALL, dsp_block="mfe", raw_samples=8000, num_filters=40), [1000, 2000, 4000], {4001: (-5, "align")}),
    # float32 general shape: the stride-10 ms graph dequantised
    "stride10_f32": (dict(SMALL, frame_stride=0.01, win_size=31, f32=True), [2399, 3999], {3840: (-5, "past")}),
}


# geometries kws_create refuses: name -> (synth_model_blob keyword arguments, code).  -18 KWS_ERROR_UNSUPPORTED_MODEL: the MFE block is
# served by tuned plans only (kws_plan.cpp: 74 frames, 24 filters and a 31-row cmvnw window are outside them); mfe_500ms covers the MFE
# class in the grid instead
CREATE_REFUSED = {
    "mfe_1500ms": (dict(SMALL, dsp_block="mfe", raw_samples=24000, num_filters=24, win_size=31), -18),
}


def model_blob(name):
    src = GRID[name][0]
    if isinstance(src, str):
        return open(os.path.join(MODELS, src), "rb").read()
    return synth_blob(src)


def synth_blob(src):
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from dequantize_model import dequantize
    from synth_model import synth_model_blob
    kw = {k: v for k, v in src.items() if k != "f32"}
    blob = synth_model_blob(seed=7, **kw)
    return dequantize(blob) if src.get("f32") else blob


def model_path(name, tmp_dir):
    """the model as a .kwsm file: the shipped file, or the synthetic one written to tmp_dir"""
    src = GRID[name][0]
    if isinstance(src, str):
        return os.path.join(MODELS, src)
    p = os.path.join(str(tmp_dir), name + ".kwsm")
    if not os.path.exists(p):
        with open(p, "wb") as f:
            f.write(model_blob(name))
    return p


def geometry(cfg, n_features):
    """(frame, stride, grow, rows, cols) of a model from its oracle MfccConfig"""
    frame = int(np.round(np.float32(FREQ) * np.float32(cfg.frame_length)))
    stride = int(np.round(np.float32(FREQ) * np.float32(cfg.frame_stride)))
    grow = int(np.float32(cfg.frame_length) * np.float32(FREQ))
    cols = cfg.num_cepstral
    return frame, stride, grow, n_features // cols, cols


class Layout:
    def __init__(self, **kw):
        self.__dict__.update(kw)

    def windows(self, n_samples):
        k = n_samples // self.slice
        return k - self.k_full if k > self.k_full else 0

    def __repr__(self):
        return "nf0/nf1 %d/%d ring_rows/rows %d/%d k_full %d keep %d grow %d" % (self.nf0, self.nf1, self.ring_rows, self.rows, self.k_full,
                                                                                 self.keep, self.grow)


def slice_walk(frame, stride, grow, rows, cols, slice_samples):
    """the reference's walk for one slicing: Layout, or the step at which the reference's frame count refuses it ('nf' rule), as an int.
    The frame count is computed as the reference does: float division of a size_t difference, floored."""
    F = rows * cols
    off, full, nf0, nf1, k_full, ring_rows = 0, False, None, None, None, None
    for k in range(4 * rows + 8):
        n_claimed = slice_samples + (grow if k > 0 else 0)
        if n_claimed < frame:
            return k
        nf = int(np.floor(np.float32(n_claimed - frame) / np.float32(stride)))
        fs = nf * cols
        if nf < 1 or fs > F or off + fs > F:
            return k
        if k == 0:
            nf0 = nf
        elif nf1 is None:
            nf1 = nf
        if full and k > k_full + 1:
            break
        if not full:
            off += fs
            if off > F - fs:
                full = True
                off -= fs
                ring_rows = (off + fs) // cols
                k_full = k
    assert full and nf1 is not None
    return Layout(slice=slice_samples, nf0=nf0, nf1=nf1, ring_rows=ring_rows, rows=rows, k_full=k_full, keep=ring_rows - nf1, grow=grow,
                  frame=frame, stride=stride)


def reads_past(lay, fft):
    """the stream API's read rule: the last frame of a grown slice must lie inside the slice (min(fft, frame) samples of it are read)"""
    return (lay.nf1 - 1) * lay.stride + min(fft, lay.frame) > lay.slice or (lay.nf0 - 1) * lay.stride + min(fft, lay.frame) > lay.slice


# the layout classes the grid must cover: name -> predicate over (model name, is generic plan, is mfe, is float32, Layout)
CLASSES = {
    "nf0 == nf1": lambda g, lay: lay.nf0 == lay.nf1,
    "nf1 - nf0 >= 2": lambda g, lay: lay.nf1 - lay.nf0 >= 2,
    "ring_rows == rows": lambda g, lay: lay.ring_rows == lay.rows,
    "ring_rows < rows": lambda g, lay: lay.ring_rows < lay.rows,
    "k_full == 0 (keep == 0)": lambda g, lay: lay.k_full == 0 and lay.keep == 0,
    "k_full >= 7": lambda g, lay: lay.k_full >= 7,
    "ring_rows % nf1 != 0": lambda g, lay: lay.ring_rows % lay.nf1 != 0,
    "grow != frame length": lambda g, lay: lay.grow != lay.frame,
    "odd slice on a generic plan": lambda g, lay: g["generic"] and lay.slice % 2 == 1,
    "MFE block": lambda g, lay: g["mfe"],
    "float32 graph": lambda g, lay: g["f32"],
}


def oracle_scan(om, rec, slice_samples, early=0):
    """scores [W][labels] of one recording through a fresh kwso_continuous (oracle/kws_oracle.c), slice by slice, each slice k >= 1 with
    the look-ahead sample the contract defines (scan_testlib.wrap_sample) -- or, with early = e, the sample e positions before it (the
    sensitivity check).  Each slice's frames may read on into the recording (kwso_continuous_step_ex): a frame longer than the FFT reads
    samples the transform drops; past the recording's end they are 0.  Returns (scores, step of the first refusal or None, its code)."""
    L = om.o.L
    grow = int(np.float32(om.cfg.frame_length) * np.float32(om.cfg.sampling_frequency))
    frame = int(np.round(np.float32(FREQ) * np.float32(om.cfg.frame_length)))
    h = L.kwso_continuous_create(om.h)
    assert h
    out, bad = [], (None, 0)
    try:
        s = np.zeros(om.n_labels, np.float32)
        produced = C.c_int()
        eos = np.zeros(1, np.float32)
        sl = np.zeros(slice_samples + frame, np.int16)
        for k in range(rec.size // slice_samples):
            seg = rec[k * slice_samples:(k + 1) * slice_samples + frame]
            sl[:] = 0
            sl[:seg.size] = seg
            p = k * slice_samples + slice_samples + (grow if k > 0 else 0) - 1 - (early if k > 0 else 0)
            eos[0] = np.float32(rec[p]) * np.float32(1.0 / 32768.0) if p < rec.size else np.float32(0.0)
            rc = L.kwso_continuous_step_ex(h, sl.ctypes.data, slice_samples, sl.size, eos.ctypes.data, s.ctypes.data, C.byref(produced))
            if rc:
                bad = (k, rc)
                break
            if produced.value:
                out.append(s.copy())
    finally:
        L.kwso_continuous_free(h)
    return np.array(out, np.float32).reshape(-1, om.n_labels), bad[0], bad[1]


def lengths_for(lay, long_s=0):
    """recording lengths around the layout's edges: shorter than a window, k_full + 1 slices +- 1 sample, the last look-ahead sample just
    outside / just inside the recording, a few slices more, optionally a long one"""
    s, kf, g = lay.slice, lay.k_full, lay.grow
    out = [0, 1, s - 1, s, (kf + 1) * s - 1, (kf + 1) * s, (kf + 1) * s + 1, (kf + 2) * s + g - 1, (kf + 2) * s + g, (kf + 5) * s + 17]
    if g >= s:                    # (the look-ahead pair must leave the slice count alone)
        out = out[:7] + out[9:]
    if long_s:
        out.append(long_s * FREQ + 123)
    return sorted(set(out))


def test_audio(oracle, lay, seed, long_s=0):
    """recordings of every length of lengths_for: speech-like, plus digital silence, DC and audio that goes silent mid-recording"""
    recs = [speech(oracle, seed * 1000 + i, n) for i, n in enumerate(lengths_for(lay, long_s))]
    n = (lay.k_full + 4) * lay.slice + lay.grow
    recs.append(np.zeros(n, np.int16))
    recs.append(np.full(n + 3, 1234, np.int16))
    r = speech(oracle, seed * 1000 + 99, n + lay.slice)
    r[n // 2:] = 0
    recs.append(r)
    return recs

