"""The MFE block at general DSP shapes (tests/mfe_general_shapes.py), without a GPU: kwso_extract_mfe -- what the GPU tests hold the kernels to --
pinned bit for bit against the compiled reference (feature::mfe of the L476 build, then cmvnw(win, false, true) + numpy::normalize of the L432
headers compiled in place), at every shape, incl. an all-zero and a constant clip whose normalisation is the reference's 0 x inf; and the
committed fixture tests/golden/mfe_general_l432.npz (tools/make_golden_mfe_general.py) against the oracle, so that a machine without the
reference checks against the reference's own numbers."""
import os

import numpy as np
import pytest

import mfe_general_shapes as G
from kws_testlib import GOLDEN, REF432_SO, OracleModel, bits


def _same_bits_or_both_nan(a, b):
    a = np.asarray(a, np.float32); b = np.asarray(b, np.float32)
    return ((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all()


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, G.FIXTURE))


@pytest.mark.parametrize("tag", sorted(G.SHAPES))
def test_oracle_extract_mfe_is_the_compiled_reference(tag, oracle, reference, tmp_path):
    from kws_testlib import ReferenceL432Dsp
    if not os.path.exists(REF432_SO):
        pytest.skip("oracle/_ref/libei_ref_l432dsp.so not built (no reference sources here)")
    r432 = ReferenceL432Dsp()
    om = OracleModel(oracle, G.write_model(tag, tmp_path))
    c = om.cfg.copy(pre_cof=0.0)
    nan = []
    for x in G.fixture_clips(oracle, tag):
        mel, _ = reference.mfe(x, c)
        assert mel.shape == G.ROWS_COLS[tag]
        want = r432.cmvnw(mel, c.win_size, False, True).reshape(-1)
        assert _same_bits_or_both_nan(want, oracle.extract_mfe(x, om.cfg)), tag
        nan.append(bool(np.isnan(want).all()))
    # the all-zero clip: every mel energy equal, range 0, 0 x inf; a window of one row: x - x everywhere, every clip
    assert nan[2] and (all(nan) if tag == "E2" else not nan[0] and not nan[1]), (tag, nan)


@pytest.mark.parametrize("tag", sorted(G.SHAPES))
def test_fixture_is_the_oracles(tag, oracle, golden, tmp_path):
    om = OracleModel(oracle, G.write_model(tag, tmp_path))
    clips = G.fixture_clips(oracle, tag)
    assert (golden[tag + "_pcm"] == clips).all()
    assert golden[tag + "_features"].shape == (G.FIXTURE_CLIPS, G.ROWS_COLS[tag][0] * G.ROWS_COLS[tag][1])
    s, f, q = om.run_batch(clips, want_features=True)
    assert _same_bits_or_both_nan(f, golden[tag + "_features"])
    assert (q == golden[tag + "_q"]).all() and (bits(s) == bits(golden[tag + "_scores"])).all()
    assert (np.isnan(f).all(axis=1) | np.isfinite(f).all(axis=1)).all()            # a clip is NaN as a whole or not at all
    assert np.isnan(f[2]).all()                                                     # the all-zero clip
    if tag == "E2":
        assert np.isnan(f).all()
    else:
        assert np.isfinite(f[:2]).all() and f[:2].min() == 0.0 and f[:2].max() <= 1.0


def test_fixture_fits_the_committed_file_limit():
    assert os.path.getsize(os.path.join(GOLDEN, G.FIXTURE)) < 1 << 20
