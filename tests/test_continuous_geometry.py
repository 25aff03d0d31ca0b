"""Continuous mode at every slicing and frame geometry of the grid (tests/continuous_geometry.py), without a GPU:
  - the grid still covers every layout class, and each refused slicing is refused for the rule it is listed with;
  - the restated slice walk gives the window count the oracle's kwso_continuous_step produces, and the oracle's windows depend on the
    look-ahead sample's position (where pre-emphasis reads it at all);
  - the host side of the three APIs (kws_scan_window_count, kws_live_window_count / a push, the stream API's steps) under ASan + UBSan
    against the stub HIP runtime of tests/sanitize: acceptance and refusal codes agree with each other and with the grid, and every window
    count agrees with the restatement."""
import glob
import os
import subprocess

import numpy as np
import pytest

import continuous_geometry as cg
from kws_testlib import ROOT, OracleModel

CSRC = os.path.join(ROOT, "ei-keyword-spotting_amd", "csrc")
CLANG = "/opt/rocm/lib/llvm/bin/clang++"
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-g", "-O1"]
# the flags of tests/sanitize/Makefile's host-only build of the library
FLAGS = ["-x", "hip", "--cuda-host-only", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-ffp-contract=off",
         "-DKWS_BUILDING_LIBRARY", "-Wno-unused-value"] + SAN
GENERIC = {"stride10", "stride10_f32", "odd_stride_fft512", "fft128_win51", "two_s_40f"}    # plans the tuned kernels do not serve whole
STEPS = 24


@pytest.fixture(scope="module")
def models(oracle, tmp_path_factory):
    """name -> (path, OracleModel, (frame, stride, grow, rows, cols))"""
    d = tmp_path_factory.mktemp("geometry_models")
    out = {}
    for name in cg.GRID:
        p = cg.model_path(name, d)
        om = OracleModel(oracle, p)
        out[name] = (p, om, cg.geometry(om.cfg, om.n_features))
    return out


def _facts(name, om):
    src = cg.GRID[name][0]
    return {"generic": name in GENERIC, "mfe": isinstance(src, dict) and src.get("dsp_block") == "mfe", "f32": "f32" in name}


def test_grid_covers_every_layout_class(models):
    found = {c: [] for c in cg.CLASSES}
    for name, (p, om, geo) in models.items():
        for sl in cg.GRID[name][1]:
            lay = cg.slice_walk(*geo, sl)
            assert isinstance(lay, cg.Layout), (name, sl, lay)
            assert not cg.reads_past(lay, om.cfg.fft_length), (name, sl, lay)
            for c, pred in cg.CLASSES.items():
                if pred(_facts(name, om), lay):
                    found[c].append("%s@%d" % (name, sl))
    missing = [c for c, v in found.items() if not v]
    assert not missing, "layout classes no grid case covers: %s" % missing
    print("\n".join("%-28s %s" % (c, ", ".join(v)) for c, v in found.items()))


def test_refusals_follow_their_rule(models):
    """each refused slicing breaks the rule it is listed with (and, for the 'nf' rule, so does the oracle's own walk)"""
    for name, (p, om, geo) in models.items():
        frame, stride, grow, rows, cols = geo
        for sl, (code, rule) in cg.GRID[name][2].items():
            lay = cg.slice_walk(*geo, sl)
            if rule == "nf":
                assert isinstance(lay, int), (name, sl)
                rec = np.zeros(sl * (lay + 2) + frame, np.int16)
                w, k, rc = cg.oracle_scan(om, rec, sl)
                assert (k, rc) == (lay, -5), (name, sl, k, rc)
                continue
            assert isinstance(lay, cg.Layout), (name, sl)
            if rule == "align":
                assert name not in GENERIC and sl % 8 != 0, (name, sl)
            elif rule == "past":
                assert cg.reads_past(lay, om.cfg.fft_length), (name, sl)
            else:
                raise AssertionError(rule)


def test_oracle_window_counts_and_look_ahead_sensitivity(models, oracle):
    """per accepted slicing: the oracle produces the restatement's window count for every test length, and reading the look-ahead sample
    one position early changes a window -- except where pre-emphasis is off (pre_cof 0, which the MFE block forces), where it must not"""
    for name, (p, om, geo) in models.items():
        insensitive = om.cfg.pre_cof == 0 or _facts(name, om)["mfe"]
        for sl in cg.GRID[name][1]:
            lay = cg.slice_walk(*geo, sl)
            recs = cg.test_audio(oracle, lay, seed=3)
            changed = False
            for r in recs:
                w, k, rc = cg.oracle_scan(om, r, sl)
                assert k is None, (name, sl, r.size, k, rc)
                assert w.shape[0] == lay.windows(r.size), (name, sl, r.size, w.shape[0], lay)
                if w.shape[0] and not changed:
                    w2, _, _ = cg.oracle_scan(om, r, sl, early=1)
                    changed = not (w2.view(np.uint32) == w.view(np.uint32)).all()
            assert changed != insensitive, (name, sl, "look-ahead position changes no window" if not changed else "pre-emphasis is off")


@pytest.fixture(scope="module")
def geometry_exe(host_exe):
    """tests/scan/geometry_host_driver.cpp linked with the host objects host_exe built, plus the scan and live units compiled the same way"""
    base = os.path.dirname(host_exe)
    out = os.path.join(base, "geometry")            # a directory of its own: the other stub tests link every object file of base
    os.makedirs(out, exist_ok=True)
    objs = []
    for unit, ext in (("kws_scan", "cpp"), ("kws_scan_kernels", "hip"), ("kws_live", "cpp"), ("kws_live_kernels", "hip")):
        o = os.path.join(out, "geo_" + unit + ".o")
        subprocess.check_call([CLANG] + FLAGS + ["-c", "-o", o, os.path.join(CSRC, unit + "." + ext)])
        objs.append(o)
    # the kernel units' host sides refer to their device code objects: one dummy word each (as tests/sanitize/Makefile does for the others)
    syms = subprocess.check_output(["nm", "-u", objs[1], objs[3]]).decode().split()
    known = open(os.path.join(base, "fatbin_syms.c")).read()
    extra = sorted({s for s in syms if s.startswith("__hip_fatbin_") and s not in known})
    src = os.path.join(out, "geo_fatbin_syms.c")
    with open(src, "w") as f:
        f.writelines("const unsigned long long %s = 0;\n" % s for s in extra)
    fo = os.path.join(out, "geo_fatbin_syms.o")
    subprocess.check_call([CLANG, "-x", "c", "-c", "-o", fo, src])
    drv = os.path.join(out, "geometry_host_driver.o")
    subprocess.check_call([CLANG, "-x", "c++", "-std=c++17"] + SAN + ["-c", "-o", drv, os.path.join(ROOT, "tests", "scan", "geometry_host_driver.cpp")])
    skip = {"host_driver.o", "boundary_driver.o", "hip_stub.o", "fatbin_syms.o"}
    lib_objs = [p for p in sorted(glob.glob(os.path.join(base, "*.o"))) if os.path.basename(p) not in skip and not os.path.basename(p).startswith("scan_")]
    exe = os.path.join(out, "kws_geometry_san")
    subprocess.check_call([CLANG] + SAN + ["-o", exe] + lib_objs + objs + [fo, os.path.join(base, "fatbin_syms.o"), os.path.join(base, "hip_stub.o"), drv,
                                                                         "-ldl", "-lpthread"])
    return exe


def _run(exe, path, slicings, lengths):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([exe, path, str(STEPS), ",".join(map(str, slicings)), ",".join(map(str, lengths))], capture_output=True, text=True,
                       env=env, timeout=600)
    assert p.returncode == 0, p.stderr[-4000:]
    r = {"slicing": {}, "count": {}}
    for line in p.stdout.splitlines():
        f = line.split()
        if f[0] == "model":
            r["rc"] = int(f[3])
        elif f[0] == "slicing":
            r["slicing"][int(f[1])] = tuple(int(x) for x in f[2:])
        elif f[0] == "count":
            r["count"][(int(f[1]), int(f[2]))] = tuple(int(x) for x in f[3:])
    return r


def test_host_counts_and_refusals_under_sanitizers(geometry_exe, models):
    for name, (path, om, geo) in models.items():
        acc, refused = cg.GRID[name][1], cg.GRID[name][2]
        lengths = sorted({n for sl in acc for n in cg.lengths_for(cg.slice_walk(*geo, sl), long_s=61)})
        r = _run(geometry_exe, path, acc + sorted(refused), lengths)
        assert r["rc"] == 0, name
        for sl in acc:
            lay = cg.slice_walk(*geo, sl)
            count_rc, scan_rc, live_rc, stream_rc, steps, produced = r["slicing"][sl]
            assert (count_rc, scan_rc, live_rc, stream_rc, steps) == (0, 0, 0, 0, STEPS), (name, sl, r["slicing"][sl])
            assert produced == lay.windows(STEPS * sl), (name, sl, produced, lay)
            for n in lengths:
                ws, wf, wo, halves, push_rc = r["count"][(sl, n)]
                want = lay.windows(n)
                assert push_rc == 0 and ws == wf == halves == want, (name, sl, n, r["count"][(sl, n)], want, lay)
                # not finished: a slice k >= 1 waits for its look-ahead sample k sl + sl + grow - 1 (slice 0 for nothing)
                done = n // sl if n < sl else max(1, (n - lay.grow) // sl if n >= lay.grow else 0)
                assert wo == lay.windows(done * sl), (name, sl, n, wo, lay)
        for sl, (code, rule) in refused.items():
            count_rc, scan_rc, live_rc, stream_rc, steps, produced = r["slicing"][sl]
            assert count_rc == scan_rc == live_rc == stream_rc == code, (name, sl, rule, r["slicing"][sl])


def test_create_refusals_under_sanitizers(geometry_exe, tmp_path):
    for name, (kw, code) in cg.CREATE_REFUSED.items():
        p = str(tmp_path / (name + ".kwsm"))
        with open(p, "wb") as f:
            f.write(cg.synth_blob(kw))
        assert _run(geometry_exe, p, [4000], [16000])["rc"] == code, name
