"""The MFE-block models of the general-shape tests (tests/test_mfe_general_pin.py, test_mfe_general_host.py, test_gpu_mfe_general.py,
tools/make_golden_mfe_general.py, tools/gpu_mfe_general_rate.py): synth_model_blob keyword arguments per shape, all 16 kHz, each the
smallest that reaches its code path.

  tag  frames x filters  what it reaches
  A    98 x 40           1 s, 20 ms frames every 10 ms, fft 256, window 101: the tuned spectral kernel over two chunks of 49 frames
  B    60 x 32           32 ms frames every 16 ms, fft 512: the cooperative kernel
  C    104 x 32          20 ms frames every 150 samples, fft 256: an unaligned stride, the cooperative kernel at fft 256
  D    38 x 64           50 ms frames every 25 ms, fft 1024, 64 filters: more columns than the tuned kernel's 40; frames shorter than the fft
  E1   49 x 32           the tuned shape with a window of 5 rows: tuned spectral kernel, general normalisation
  E2   49 x 32           ... of 1 row: pad 0, every output x - x, the whole matrix NaN after the scale
  F    188 x 64          2 s, 20 ms frames every 168 samples, window 151: the global-memory form of the normalisation (135 KB padded + outputs)
"""
import os
import sys

import numpy as np

from kws_testlib import ROOT

def NET(p1, p2):            # two conv blocks whose pools divide the frame count (SAME pooling with padding is outside the network kernels)
    return dict(blocks=((8, 3, p1), (4, 3, p2)), n_labels=3, dsp_block="mfe")



SHAPES = {
    "A": dict(NET(7, 7), seed=101, num_filters=40, high=0, frame_stride=0.01),
    "B": dict(NET(6, 5), seed=102, fft_length=512, frame_length=0.032, frame_stride=0.016),
    "C": dict(NET(8, 1), seed=103, frame_stride=150 / 16000.0),
    "D": dict(NET(2, 1), seed=104, num_filters=64, high=0, fft_length=1024, frame_length=0.05, frame_stride=0.025),
    "E1": dict(NET(7, 7), seed=105, win_size=5),
    "E2": dict(NET(7, 7), seed=106, win_size=1),
    "F": dict(NET(4, 1), seed=107, num_filters=64, high=0, raw_samples=32000, frame_stride=168 / 16000.0, win_size=151),
}
ROWS_COLS = {"A": (98, 40), "B": (60, 32), "C": (104, 32), "D": (38, 64), "E1": (49, 32), "E2": (49, 32), "F": (188, 64)}
# what kws_mfcc_kernel_name reports, and the form of the normalisation
SPECTRAL = {"A": "kws_mfcc8_kernel (chunked)", "B": "kws_spectral_lds_kernel", "C": "kws_spectral_lds_kernel", "D": "kws_spectral_lds_kernel",
            "E1": "kws_mfcc8_kernel (chunked)", "E2": "kws_mfcc8_kernel (chunked)", "F": "kws_spectral_lds_kernel"}
NORM_LDS = {"A": True, "B": True, "C": True, "D": True, "E1": True, "E2": True, "F": False}
# an fft whose half needs radix 7: kf_bfly_generic is not restated, MFE block or not
RADIX7_KW = dict(NET(1, 1), seed=108, fft_length=448, frame_length=0.028, frame_stride=0.014)
# a general MFE plan is admitted from 32 filters up (the counts pinned against the compiled reference); below, it stays refused
FEW_FILTERS_KW = dict(NET(1, 1), seed=109, num_filters=24, raw_samples=24000, win_size=31)
FIXTURE = "mfe_general_l432.npz"
FIXTURE_CLIPS = 4             # per shape: two synthetic clips (seed 17, from clip 0), the all-zero clip and a constant one


def blob(tag, f32=False):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from dequantize_model import dequantize
    from synth_model import synth_model_blob
    b = synth_model_blob(**(SHAPES[tag] if isinstance(tag, str) else tag))
    return dequantize(b) if f32 else b


def write_model(tag, tmp_dir, f32=False):
    p = os.path.join(str(tmp_dir), "mfe_%s%s.kwsm" % (tag, "_f32" if f32 else ""))
    if not os.path.exists(p):
        with open(p, "wb") as f:
            f.write(blob(tag, f32))
    return p


def fixture_clips(oracle, tag):
    n = SHAPES[tag].get("raw_samples", 16000)
    return np.concatenate([oracle.synth(17, 0, FIXTURE_CLIPS - 2, clip_len=n), np.zeros((1, n), np.int16), np.full((1, n), 1234, np.int16)])
