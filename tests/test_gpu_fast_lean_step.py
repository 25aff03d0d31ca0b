"""-m gpu: the fast kernel's spectral pass after it shed its exact no-ops -- the power rows are unscaled (the plan's mel tap weights carry the power of two,
the frame energy takes it once; csrc/kws_fast_scale.h) and the m = 2, k = 1 butterflies use their twiddles' structure (csrc/kws_bfly_m2k1.h) -- in every
form that runs the pass loop on a shipped graph: the headline 49x40 float32 graph and its 49x13 twin (three waves per SIMD, clips by ticket, paired tail
pass) and the 49x40 int8 graph (two waves per SIMD, the int8 network in the same launch).

Both changes are identities, so the bars are the ones that stood before: float32 scores within 1e-4 of the oracle's (BASELINE's north star, the bar of
test_gpu_fast_mode.py); the int8 graph is exact from its input tensor on, so its bar is test_gpu_fast_mode.py's as well -- at most 2 % of the synthetic clips
with a changed score.  Inputs: the bench's synthetic clips at batch sizes one below, at and one above the grid's wave count (every wave one clip; a few waves a
second one; the tail pass with and without a partner) and B = 1, and 256 hard clips (bursts, a word followed by digital silence: frames whose power rows are
exactly zero, where the moved scale must still meet the == 0 tests with the same value) of which the guard hands some on to the exact kernels.

A handle's calls in a row -- friendly, hard and single-clip batches mixed, with and without a host synchronisation between them -- must each give the bits and
the two counts (kws_fast_fallback_count, kws_fast_exact_count) of a FRESH handle that was given only that one call: the kernels' results do not depend on
which wave takes which clip, nor on what the handle ran before."""
import multiprocessing as mp
import os

import numpy as np
import pytest

from kws_families import family, word_waveforms
from kws_testlib import MODELS, ROOT, Oracle, OracleModel, bits

pytestmark = pytest.mark.gpu

FAST_SCORE_TOL = 1e-4
N_HARD = 256
MODEL_NAMES = ("cfg2_mfcc40_f32.kwsm", "l476_no_yes_f32.kwsm", "cfg2_mfcc40_int8.kwsm")


@pytest.fixture(scope="module")
def pkg():
    import sys
    sys.path.insert(0, ROOT)
    import torch  # noqa: F401
    from __graft_entry__ import load_package
    return load_package()


_W = {}


def _oracle_worker(args):
    path, pcm = args
    if path not in _W:
        _W[path] = OracleModel(_W.setdefault("oracle", Oracle()), path)
    return _W[path].run_batch(pcm)


@pytest.fixture(scope="module")
def pool():
    with mp.get_context("spawn").Pool(min(16, len(os.sched_getaffinity(0)))) as p:
        yield p


class Bench:
    """One model's inputs (on the device), the fresh-handle results of every distinct call (made once, kept unchanged) and the oracle's scores."""

    def __init__(self, pkg, name, hard_host, pool):
        import torch
        self.pkg, self.name, self.path = pkg, name, os.path.join(MODELS, name)
        gm = pkg.Model(self.path, device=0)
        tol = gm.fast_tolerance()
        self.is_float, self.n_labels, self.n_features = bool(gm.is_float), gm.n_labels, gm.n_features
        # waves of a full grid: 256 workgroups x the plan's waves (float32: 11 / 12 at three waves per SIMD; the int8 form: at most eight at two)
        self.waves = 256 * (tol["fused_waves"] if self.is_float else 8)
        # the route under test: batch calls start in the fast kernel (first tier), the float32 graphs in the three-wave build
        assert tol["entry_tier"] == 1 and (not self.is_float or tol["fused_waves_per_simd"] == 3), tol
        gm.close()
        easy_host = Oracle().synth(0, 0, self.waves + 1)                        # the bench's synthetic clips
        self.host = {"easy": easy_host, "hard": hard_host}
        self.dev = {k: torch.from_numpy(v).to("cuda:0") for k, v in self.host.items()}
        self.oracle = {k: np.concatenate(pool.map(_oracle_worker, [(self.path, v[i:i + 128]) for i in range(0, len(v), 128)])) for k, v in self.host.items()}
        self.fresh = {}

    def pcm(self, what):
        src, n = what
        return self.dev[src][:n].contiguous()

    def call(self, gm, kind, what):
        """one call on handle gm, nothing read back: -> dict of device tensors.  kind: batch (scores: the fused forms) | batch_f (the feature matrix too -- and an
        int8 graph's input tensor --: the feature-emitting forms run the same pass loop)"""
        import torch
        pcm = self.pcm(what)
        n = pcm.shape[0]
        out = {"scores": torch.full((n, self.n_labels), float("nan"), dtype=torch.float32, device="cuda:0")}
        if kind == "batch_f":
            out["features"] = torch.full((n, self.n_features), float("nan"), dtype=torch.float32, device="cuda:0")
            if not self.is_float:
                out["q"] = torch.zeros((n, self.n_features), dtype=torch.int8, device="cuda:0")
        elif kind != "batch":
            raise ValueError(kind)
        f, q = out.get("features"), out.get("q")
        gm.run_classifier_batch_device(pcm.data_ptr(), n, out["scores"].data_ptr(), None if f is None else f.data_ptr(), None if q is None else q.data_ptr())
        return out

    @staticmethod
    def read(out):
        return {k: v.cpu().numpy() for k, v in out.items()}

    def reference(self, kind, what):
        """the same call on a fresh handle that sees nothing else: outputs and both counts"""
        import torch
        key = (kind, what)
        if key not in self.fresh:
            gm = self.pkg.Model(self.path, device=0)
            gm.set_mode(self.pkg.MODE_FAST)
            out = self.call(gm, kind, what)
            torch.cuda.synchronize()
            res = self.read(out)
            res["counts"] = (gm.fast_fallback_count(), gm.fast_exact_count())
            gm.close()
            for v in res.values():
                if isinstance(v, np.ndarray):
                    v.setflags(write=False)
            self.fresh[key] = res
        return self.fresh[key]

    def check(self, got, counts, kind, what, where):
        ref = self.reference(kind, what)
        for k, v in got.items():
            assert not np.isnan(v).any(), (self.name, where, k)
            assert (bits(v) == bits(ref[k])).all(), "%s, %s: %s differs from a fresh handle's in %d values" % (self.name, where, k, int((bits(v) != bits(ref[k])).sum()))
        if counts is not None:
            assert counts == ref["counts"], "%s, %s: (handed on, ended in the exact kernels) = %s, a fresh handle's %s" % (self.name, where, counts, ref["counts"])

    def run_sequence(self, seq, sync_between=True):
        """seq: [(kind, what)], all on ONE handle.  sync_between: read outputs and counts after every call; else enqueue everything, synchronise once, compare
        every call's outputs and the last call's counts"""
        import torch
        gm = self.pkg.Model(self.path, device=0)
        gm.set_mode(self.pkg.MODE_FAST)
        pending = []
        for i, (kind, what) in enumerate(seq):
            out = self.call(gm, kind, what)
            where = "call %d of %s" % (i, [k + ":" + w[0] + str(w[1]) for k, w in seq])
            if sync_between:
                torch.cuda.synchronize()
                self.check(self.read(out), (gm.fast_fallback_count(), gm.fast_exact_count()), kind, what, where)
            else:
                pending.append((out, kind, what, where))
        if not sync_between:
            torch.cuda.synchronize()
            counts = (gm.fast_fallback_count(), gm.fast_exact_count())
            for j, (out, kind, what, where) in enumerate(pending):
                self.check(self.read(out), counts if j == len(pending) - 1 else None, kind, what, where)
        gm.close()


@pytest.fixture(scope="module")
def hard_clips(pkg):
    """128 clips of bursts and 128 of a word followed by digital silence (tests/kws_families.py): the inputs the guard hands on most often"""
    import torch
    n = N_HARD // 2
    w, ln = word_waveforms(n, 41)
    words, lens = torch.from_numpy(w).to("cuda:0"), torch.from_numpy(ln).to("cuda:0")
    out = torch.zeros((n, 16000), dtype=torch.int16, device="cuda:0")
    pkg.mix_audio_device(words.data_ptr(), lens.data_ptr(), 16000, None, 0, None, 1.0, 0.0, n, 16000, out.data_ptr())
    torch.cuda.synchronize()
    return np.ascontiguousarray(np.concatenate([family("bursts", n, seed=42), out.cpu().numpy()]))


_BENCHES = {}


@pytest.fixture(params=MODEL_NAMES)
def bench(request, pkg, hard_clips, pool):
    if request.param not in _BENCHES:
        _BENCHES[request.param] = Bench(pkg, request.param, hard_clips, pool)
    return _BENCHES[request.param]


def sizes(b):
    w = b.waves
    return ("easy", w - 1), ("easy", w), ("easy", w + 1), ("hard", N_HARD), ("easy", 1)


def test_single_calls_meet_the_fast_modes_bar_and_hand_on_what_they_should(bench):
    """the references themselves: the friendly batch hands nothing on (float32 graphs: pinned by test_gpu_fast_cmvn_store.py), the hard one many; scores against the oracle"""
    below, at, above, hard, one = sizes(bench)
    for what in (above, hard):
        ref = bench.reference("batch", what)
        so = bench.oracle[what[0]][:what[1]]
        d = np.abs(ref["scores"] - so)
        print("\n%s %s x %d: max |score - oracle| = %.3g, handed on %d, ended in the exact kernels %d" % ((bench.name,) + what + (d.max(),) + ref["counts"]))
        if bench.is_float:
            assert d.max() <= FAST_SCORE_TOL
        elif what[0] == "easy":
            assert (d.max(axis=1) > 0).mean() <= 0.02
        if what[0] == "hard":
            assert 0 < ref["counts"][0] <= N_HARD and ref["counts"][1] <= ref["counts"][0]      # the sequences below need a list that is NOT empty
        elif bench.is_float:
            assert ref["counts"] == (0, 0)


@pytest.mark.parametrize("sync_between", [True, False], ids=["sync", "nosync"])
def test_batch_calls_in_a_row(bench, sync_between):
    below, at, above, hard, one = sizes(bench)
    bench.run_sequence([("batch", at), ("batch", hard), ("batch", below), ("batch_f", hard), ("batch", one), ("batch", above), ("batch_f", at), ("batch", hard), ("batch", at)],
                       sync_between)
