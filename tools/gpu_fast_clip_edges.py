"""Development aid: what the three-waves-per-SIMD fast kernel waits for at a clip's edge -- shader clocks of phase 0 (samples to butterfly inputs, the next
pass's requests) of every clip's PASS 0, from the pass's top, against the same phase of the clip's other passes, for wave 0 of workgroup 0 of a full launch
(the PROF form's slots 16 .. 18, csrc/kws_fast.hip).  Pass 0 is the one pass whose samples were requested a moment, not a pass, before they are used: the
difference is what a clip's cold start costs the wave.

    python tools/gpu_fast_clip_edges.py [model.kwsm] [clips = 65536] [kernel microseconds, for the last line]
    KWS_LIB=ab_tmp/libkws_<name>.so python tools/gpu_fast_clip_edges.py ...       (another build of the library, as tools/ab_rate.py runs them)

The clocks are the PROF form's, whose register allocation is not the product form's: read the difference and its share, not the totals."""
import ctypes, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from __graft_entry__ import load_package
pkg = load_package()
path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "models", "cfg2_mfcc40_f32.kwsm")
m = pkg.Model(path)
B = int(sys.argv[2]) if len(sys.argv) > 2 else 65536
kernel_us = float(sys.argv[3]) if len(sys.argv) > 3 else 0.0
pcm = torch.empty((B, 16000), dtype=torch.int16, device="cuda")
pkg.synth_clips_device(0, 0, B, 16000, pcm.data_ptr())
s = torch.empty((B, m.n_labels), dtype=torch.float32, device="cuda")
prof = torch.zeros(24, dtype=torch.int64, device="cuda")
L = pkg.lib()
L.kws_dev_fast_phase_profile.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p]
rows = []
for _ in range(5):
    rc = L.kws_dev_fast_phase_profile(m.h, pcm.data_ptr(), B, s.data_ptr(), prof.data_ptr())
    torch.cuda.synchronize()
    rows.append(prof.cpu().numpy().copy())
tol = m.fast_tolerance()
n_frames = m.n_frames
n_tail = n_frames & 7 if n_frames >= 8 and 0 < (n_frames & 7) <= 2 else 0
n_pass = n_frames // 8 if n_tail else (n_frames + 7) // 8
print(os.path.basename(path), "rc", rc, "clips", B, "waves per SIMD", tol.get("fused_waves_per_simd"), "waves per workgroup", tol.get("fused_waves"), "passes per clip", n_pass,
      "library", os.path.basename(os.environ.get("KWS_LIB", "libkws_mi355x.so")))
if tol.get("fused_waves_per_simd") != 3:
    sys.exit("the plan is not laid out for three waves per SIMD: slots 16 .. 18 are not written")
for i, pa in enumerate(rows[1:]):            # (the first launch pays the code's own first fetch)
    clips, first, rest, total = int(pa[17]), int(pa[18]), int(pa[16]), int(pa[:9].sum())
    if clips == 0 or n_pass < 2:
        sys.exit("wave 0 took no clip, or the clip has one pass")
    per_first, per_rest = first / clips, rest / (clips * (n_pass - 1))
    excess = (per_first - per_rest) * clips
    line = "launch %d: wave 0 took %d clips; phase 0 of pass 0: %.0f clocks, of the other passes: %.0f; cold start %.0f clocks per clip = %.2f %% of the wave's clocks" % (
        i + 1, clips, per_first, per_rest, per_first - per_rest, 100.0 * excess / total)
    if kernel_us:
        line += " = %.1f us of a %.0f us launch" % (kernel_us * excess / total, kernel_us)
    print(line)
