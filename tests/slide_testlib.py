"""Helpers of the sliding one-shot window tests (kws_slide_*): the test recordings, the windows cut out on the CPU, a brute-force count
of the frame positions a recording's windows need, and the call itself with sentinel-filled margins."""
import numpy as np

from scan_testlib import pack, speech

# the MFE-block graph of tests/test_gpu_scan.py / tests/test_gpu_mfe_model.py: no shipped model uses that block
MFE_KW = dict(seed=77, blocks=((8, 3, 7), (4, 3, 7)), n_labels=3, dsp_block="mfe")
SENTINEL = -7.0
MARGIN = 3                     # rows past the last window that a call must leave alone


def brute_force_rows(n_windows, hop, stride, n_frames, pre):
    """distinct sample positions at which the frames f >= pre of windows 0 .. n_windows - 1 start: the cepstral rows that do not depend on
    the window (pre = 1: pre-emphasis blocks, frame 0 wraps to the window's own last sample; pre = 0: MFE block)"""
    if n_windows == 0:
        return 0
    w = np.arange(n_windows, dtype=np.int64)[:, None] * hop
    f = np.arange(pre, n_frames, dtype=np.int64)[None, :] * stride
    return int(np.unique(w + f).size)


def recordings(oracle, clip, hop, seed=1):
    """lengths around every edge of the window count, speech-like audio, digital silence and audio that goes silent midway; the long
    recording is left out where the hop makes its windows many (hop < 100: nothing longer than clip + 60 samples)"""
    small = hop < 100
    lengths = [0, clip - 1, clip, clip + 1, clip + hop - 1, clip + hop, clip + 3 * hop + 7, clip + 60 if small else 3 * 16000]
    recs = [speech(oracle, seed * 100 + i, n) for i, n in enumerate(lengths)]
    recs.append(np.zeros(clip + (20 if small else 2 * hop + 5), np.int16))                   # digital silence
    r = speech(oracle, seed * 100 + 40, clip + (40 if small else 3 * hop + 11))              # goes silent midway
    r[clip // 2 + 1111:] = 0
    recs.append(r)
    return recs


def n_speech_like(recs):
    """the recordings above that are speech from end to end (the first eight)"""
    return 8


def cut_windows(recs, clip, hop):
    """[sum W][clip] int16: every window of every recording, in the call's order; and W per recording"""
    W = [0 if r.size < clip else (r.size - clip) // hop + 1 for r in recs]
    rows = [r[w * hop:w * hop + clip] for r, n in zip(recs, W) for w in range(n)]
    return (np.stack(rows) if rows else np.zeros((0, clip), np.int16)), W


def slide(gm, d_pcm, offs, lens, hop, flags, want_features=True):
    """(scores [n][labels], features [n][F] or None, n) of one call; asserts that the rows behind the last window were left alone"""
    import torch
    n = sum(gm.slide_window_count(int(x), hop) for x in lens)
    s = torch.full((n + MARGIN, gm.n_labels), SENTINEL, dtype=torch.float32, device="cuda")
    f = torch.full((n + MARGIN, gm.n_features), SENTINEL, dtype=torch.float32, device="cuda") if want_features else None
    gm.slide_recordings_device(d_pcm.data_ptr(), offs, lens, hop, s.data_ptr(), f.data_ptr() if want_features else None, flags=flags)
    torch.cuda.synchronize()
    s = s.cpu().numpy()
    assert (s[n:] == SENTINEL).all(), "scores written past the last window"
    if want_features:
        f = f.cpu().numpy()
        assert (f[n:] == SENTINEL).all(), "features written past the last window"
        f = f[:n]
    return s[:n], f, n


def batch_device(gm, windows, piece=4096):
    """(scores, features) of the product's own kws_run_classifier_batch_device on windows [n][clip] (numpy or a CUDA tensor), in pieces"""
    import torch
    n = windows.shape[0]
    s = torch.empty((max(n, 1), gm.n_labels), dtype=torch.float32, device="cuda")
    f = torch.empty((max(n, 1), gm.n_features), dtype=torch.float32, device="cuda")
    for i0 in range(0, n, piece):
        w = windows[i0:i0 + piece]
        d = torch.from_numpy(np.ascontiguousarray(w)).cuda() if isinstance(w, np.ndarray) else w.contiguous()
        gm.run_classifier_batch_device(d.data_ptr(), d.shape[0], s[i0:].data_ptr(), f[i0:].data_ptr())
        torch.cuda.synchronize()
    return s[:n], f[:n]


__all__ = ["MFE_KW", "SENTINEL", "MARGIN", "brute_force_rows", "recordings", "n_speech_like", "cut_windows", "slide", "batch_device", "pack", "speech"]
