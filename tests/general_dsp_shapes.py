"""The MFCC models that walk the whole range of DSP shapes build_dsp_plan (csrc/kws_plan.cpp) hands to the general kernels of
csrc/kws_generic.hip, shared by the CPU pin (tests/test_oracle_vs_reference.py::test_general_envelope_shapes_pinned), the host routing test
(tests/test_general_envelope_host.py) and the GPU tests (tests/test_gpu_general_envelope.py, two cases of tests/test_gpu_generic_dsp.py).
Each entry: synth_model_blob keyword arguments, the kws_mfcc_kernel_name the plan must report and the form of cmvnw a batch call must
launch.  Everything is 16 kHz, 1 s clips, 20 ms frames every 20 ms (49 frames), 32 filters 300 .. 4000 Hz, 13 cepstra, window 101 and the
small network NET unless the entry says otherwise; each entry is the smallest shape that reaches its path.

  mixed-radix FFT on the cooperative kernel (kws_spectral_lds_kernel; the suite's other shapes are all powers of two)
    fft60      half 30 = 2 3 5          no radix 4; a radix-3 level of m = 5 (twiddles other than 1); truncated frames
    fft96      half 48 = 4 4 3          radix 3 at the leaves (m = 1); truncated frames
    fft320     half 160 = 4 4 2 5       radix 5 at the leaves (m = 1); the frame neither padded nor cut
    fft600     half 300 = 4 3 5 5       radix 3 of m = 25 and radix 5 of m = 5; above 512: the two-wave build (the four-wave build holds four
                                        sample dwords per lane and frame: no pair loads there)
    fft1000    half 500 = 4 5 5 5       radix 5 of m = 25 and m = 5
    (a leaf-level butterfly multiplies by twiddle 0 only: a wrong twiddle index in kf_bfly3 / kf_bfly5 shows at fft60 / fft600 / fft1000 and in the
    DCTs of 50 and 100 filters, not at fft96 / fft320 -- measured with the first two twiddles of z_bfly_one's radix-5 branch swapped)
    fft64                               the smallest power of two tests/generic_soak.py draws
  degenerate transforms: one butterfly level, 1 .. 3 split pairs, three to seven bins for 32 filters (most filters have no tap: the `+4`
  batch reads of the mel loop, the log of empty filters)
    fft4 fft6 fft10 fft12               halves 2, 3, 5, 6
  upper end
    fft2048                             the largest layout kws_generic_uses_lds admits
    fft4096                             kws_spectral_generic_kernel (scratch in HBM) by the library's own rule
  filters (the DCT's radices, and the counts above 64), all 0 .. 8000 Hz
    filters2                            a DCT over ONE complex point: kf_factor hands kf_work the "radix" 1
    filters4 filters6                   halves 2 and 3; all cepstra, so columns past NF / 2 (the transform never writes them)
    filters50 filters60                 halves 25 = 5 5 and 30 = 2 3 5
    filters72 filters100 filters128
    filters128_ncep128_fft1024          every column of the widest matrix ((49 + 100) rows x 128 columns = 76 KB: cmvnw in global memory here too)
    ncep1                               c0 alone
  cmvnw
    win1                                pad 0: every value normalised over itself -- all features are ONE value (the exception to MIN_DISTINCT)
    win3
    win301                              on 49 frames: symmetric padding several times the matrix
    cmvn_global                         64 x 64, 2 s, 10 ms stride, window 101: (198 + 100) rows x 64 columns = 76 KB > the 64 KB LDS rule of
                                        kws_launch_cmvn_generic: kws_cmvn_generic_kernel
    (win1 / win3 / win301 are fft 256, 32 filters: the tuned spectral kernel over one chunk of 49 frames, "kws_mfcc8_kernel (chunked)")
  odd geometry
    fft96_clip15999                     an odd clip length: the per-sample fetch (no dword pairs)
    fft320_odd_stride                   321-sample frames every 161 samples: likewise

What keeps a comparison over these shapes from passing vacuously (asserted where it is cheap, in the CPU pin; the GPU test asserts the
finiteness again and compares every word):
  * the oracle's features of every clip the tests use are finite at every shape: no clip is masked out, no NaN tolerated;
  * every synthetic clip's oracle feature matrix takes at least MIN_DISTINCT distinct values (the smallest measured: 50 of 637 words at fft 4),
    except win1, whose features are one value by construction -- its checks are the cepstra before cmvnw and the feature bits;
  * every served entry names its kernel: a shape that takes another one fails, it does not skip.
"""
import os

import numpy as np

from kws_testlib import special_clips, synth_model_blob

NET = dict(blocks=((8, 3, 1), (4, 3, 1)), n_labels=3)
LDS, SCRATCH, CHUNKED = "kws_spectral_lds_kernel", "kws_spectral_generic_kernel", "kws_mfcc8_kernel (chunked)"
WIDE = dict(low=0, high=0)

# name: (synth_model_blob arguments, kws_mfcc_kernel_name, cmvnw in LDS?)
SERVED = {
    "fft60": (dict(fft_length=60), LDS, True),
    "fft96": (dict(fft_length=96), LDS, True),
    "fft320": (dict(fft_length=320), LDS, True),
    "fft600": (dict(fft_length=600), LDS, True),
    "fft1000": (dict(fft_length=1000), LDS, True),
    "fft64": (dict(fft_length=64), LDS, True),
    "fft4": (dict(fft_length=4), LDS, True),
    "fft6": (dict(fft_length=6), LDS, True),
    "fft10": (dict(fft_length=10), LDS, True),
    "fft12": (dict(fft_length=12), LDS, True),
    "fft2048": (dict(fft_length=2048), LDS, True),
    "fft4096": (dict(fft_length=4096), SCRATCH, True),
    "filters2": (dict(WIDE, num_filters=2, ncep=2), LDS, True),
    "filters4": (dict(WIDE, num_filters=4, ncep=4), LDS, True),
    "filters6": (dict(WIDE, num_filters=6, ncep=6), LDS, True),
    "filters50": (dict(WIDE, num_filters=50), LDS, True),
    "filters60": (dict(WIDE, num_filters=60), LDS, True),
    "filters72": (dict(WIDE, num_filters=72), LDS, True),
    "filters100": (dict(WIDE, num_filters=100), LDS, True),
    "filters128": (dict(WIDE, num_filters=128), LDS, True),
    "filters128_ncep128_fft1024": (dict(WIDE, num_filters=128, ncep=128, fft_length=1024), LDS, False),
    "ncep1": (dict(WIDE, num_filters=20, ncep=1), LDS, True),
    "win1": (dict(win_size=1), CHUNKED, True),
    "win3": (dict(win_size=3), CHUNKED, True),
    "win301": (dict(win_size=301), CHUNKED, True),
    "cmvn_global": (dict(WIDE, num_filters=64, ncep=64, raw_samples=32000, frame_stride=0.01), LDS, False),
    "fft96_clip15999": (dict(fft_length=96, raw_samples=15999), LDS, True),
    "fft320_odd_stride": (dict(fft_length=320, frame_length=0.0200625, frame_stride=0.0100625), LDS, True),
}
NAMES = sorted(SERVED)
# the build of the cooperative kernel a plain batch call must take where the launch rule says so outright (fft above 512: two waves per SIMD);
# everywhere else the LDS a wave needs decides, and the host routing test only asks that both builds occur in the table
TWO_WAVE = ("fft600", "fft1000", "fft2048", "filters128_ncep128_fft1024")
# int16 batches of these are fetched sample by sample (an odd clip length / an odd stride); every other cooperative shape up to fft 1024 takes dword pairs
NO_PAIRS = ("fft96_clip15999", "fft320_odd_stride", "fft2048")
# KWS_ERROR_UNSUPPORTED_MODEL: name -> (arguments, a piece of kws_last_error's text)
REFUSED = {
    "filters26": (dict(WIDE, num_filters=26), "radix other than 2, 3, 4, 5"),                # half 13
    "fft448": (dict(fft_length=448), "radix other than 2, 3, 4, 5"),                         # half 224 = 4 4 2 7
    "filters31": (dict(WIDE, num_filters=31), "filters 31"),                                 # an odd filter count
    "win100": (dict(win_size=100), "win 100"),                                               # an even cmvnw window
}
# the forms a development switch forces at small shapes (one fresh process each: the switches are read once per process)
FORCED_SCRATCH = ("fft96", "fft600", "filters100")
FORCED_CMVN_GLOBAL = ("win3", "win301", "filters128_ncep128_fft1024")            # (the last one is in global memory whatever the switch says)
FLOAT_PCM = ("fft96", "fft600", "filters100")

MIN_DISTINCT = 32
ONE_VALUE = ("win1",)
SPECIAL = ("impulses", "ramp", "zeros", "alternating_fullscale")


def kwargs(name):
    table = SERVED if name in SERVED else REFUSED
    return dict(NET, seed=7, **table[name][0])


def blob(name):
    return synth_model_blob(**kwargs(name))


def write_model(name, tmp_dir):
    p = os.path.join(str(tmp_dir), "envelope_%s.kwsm" % name)
    if not os.path.exists(p):
        with open(p, "wb") as f:
            f.write(blob(name))
    return p


def clips(oracle, n_samples, n_synth):
    """n_synth synthetic clips of the model's length, then SPECIAL resized to it"""
    sp = special_clips()
    return np.ascontiguousarray(np.concatenate([oracle.synth(5, 0, n_synth, n_samples), np.stack([np.resize(sp[k], n_samples) for k in SPECIAL])]))
