#!/usr/bin/env python3
"""Generate tests/golden/mfe_general_l432.npz from the UNMODIFIED reference compiled by `make -C oracle ref`: MFE-block models at the
general DSP shapes of tests/mfe_general_shapes.py, composed from the reference's own leaves as tools/make_golden.py composes
mfe_model_l432.npz -- extract_mfe_features = feature::mfe of the L476 build on the raw signal (the same text in both SDK copies), then
cmvnw(win, false, true) + numpy::normalize of the L432 headers compiled in place; the input quantisation; the graph through the reference's
op registrations.  Per shape: the clips of mfe_general_shapes.fixture_clips (two synthetic, the all-zero clip, a constant one) as
`<tag>_pcm`, and `<tag>_features` [clips][frames x filters], `<tag>_q` (int8 input tensor), `<tag>_scores`.

Runs only where the compiled reference exists.  A clip whose feature matrix is NaN (0 x inf of a constant clip) keeps its NaN features; its
int8 tensor and scores are what the restated input quantisation makes of them through the reference's graph."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
from kws_testlib import GOLDEN, Oracle, OracleModel, Reference, ReferenceL432Dsp  # noqa: E402
import mfe_general_shapes as G  # noqa: E402


def main():
    ref, r432, oracle = Reference(), ReferenceL432Dsp(), Oracle()
    out = {"tags": np.array(sorted(G.SHAPES))}
    for tag in sorted(G.SHAPES):
        blob = G.blob(tag)
        tmp = os.path.join(GOLDEN, "_mfe_general_tmp.kwsm")
        open(tmp, "wb").write(blob)
        om = OracleModel(oracle, tmp)                      # only for the DSP settings and the input quantisation / output dequantisation leaves
        os.remove(tmp)
        c = om.cfg.copy(pre_cof=0.0)
        clips = G.fixture_clips(oracle, tag)
        feats, qs, scores = [], [], []
        for x in clips:
            mel, _ = ref.mfe(x, c)
            assert mel.shape == G.ROWS_COLS[tag], (tag, mel.shape)
            f = r432.cmvnw(mel, c.win_size, False, True).reshape(-1)
            q = om.quantize_input(f)
            o, _ = ref.graph_run(blob, q)
            feats.append(f); qs.append(q); scores.append(om.dequantize(o))
        out[tag + "_pcm"] = clips
        out[tag + "_features"] = np.stack(feats)
        out[tag + "_q"] = np.stack(qs)
        out[tag + "_scores"] = np.stack(scores)
    path = os.path.join(GOLDEN, G.FIXTURE)
    np.savez_compressed(path, **out)
    print(G.FIXTURE, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
