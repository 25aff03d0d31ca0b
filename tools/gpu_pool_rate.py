#!/usr/bin/env python3
"""What pool calls (kws_pool_*; include/kws/kws.h) cost beside the routed bank calls a many-tenant caller had before, on one MI355X.

Tenants are synthetic int8 graphs of the stock two-block shape at 49 x 40 features (tools/synth_model.py: one seed each, 3 / 4 / 6 labels in
turn, the DSP block of models/cfg2_mfcc40_int8.kwsm), written once to --tenants and loaded from there.  Workloads (--workloads picks among
them), every variant in the same process and library, all KWS_MODE_EXACT (pool and bank calls always are):
  batch16   --clips resident clips, 16 tenants, clip i -> tenant i mod 16:
              pool   one kws_pool_run_classifier_device call
              bank   one kws_bank_run_classifier_routed_device call on the same batch and handles, one-hot routes
            BAR 1: the pool call's median must not exceed the bank call's by more than the spread between the latter's repeats.
  live256   --streams live streams of 256 tenants (streams / 256 each), one slice of 4000 samples (250 ms) per push, in steady state:
              pool   one push of one pool session
              banks  sixteen routed-bank pushes back to back on one stream: 16 banks of 16 members with streams / 16 streams each
            BAR 2: the pool push's median plus the spread between its repeats must stay below the sixteen pushes' median.
  batch256  recorded only: the same clips with 256 tenants, `even` (clip i -> tenant i mod 256) and `half` (tenant 0 holds every second
            clip, the others share the rest)
  handles   recorded only: seconds of kws_create and device bytes per tenant handle while the 256 handles are made
  items     recorded only, on the DEVELOPMENT library (its KWS_DEV_POOL_ITEM_ROWS switch): batch16, batch256 even / half and the live256
            pool push at each candidate of --item-rows, and small_one: --small clips that all name one tenant
Every variant: --warmup untimed steps, then --steps steps between two device events; the variants of one workload alternate, --repeats
times; every repeat is reported, with the median and the spread (max - min).  Before anything is timed the pool's rows are compared with the
other variant's rows of the same (row, member) pairs: they must be the same bits.  The process ends with status 1 when a bar is missed.
Each workload runs under its own time limit (--limit seconds: the process ends there, starting nothing more).  One JSON line per (workload,
variant), appended to --out; --md FILE writes the tables from --out's lines (no GPU needed for that step).

usage: gpu_pool_rate.py [--workloads batch16,live256,batch256,handles] [--clips 65536] [--streams 1024] [--out FILE.jsonl]
       gpu_pool_rate.py --workloads items [--item-rows 4,8,16,32,64] --out FILE.jsonl
       gpu_pool_rate.py --make-tenants                 (host only: writes the tenant files)
       gpu_pool_rate.py --md profiles/pool_rate.md --out FILE.jsonl
"""
import argparse
import json
import os
import signal
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

SLICE, TENANTS, BANK = 4000, 256, 16
LABELS = (3, 4, 6)
POOL_NONE = 0xffffffff


class StepLimit:
    """ends the process when the block takes longer than `seconds`: nothing more is started on the GPU after that"""

    def __init__(self, what, seconds):
        self.what, self.seconds = what, seconds

    def __enter__(self):
        def out_of_time(*_):
            print("%s: over its limit of %d s" % (self.what, self.seconds), file=sys.stderr, flush=True)
            os._exit(124)
        signal.signal(signal.SIGALRM, out_of_time)
        signal.alarm(self.seconds)

    def __exit__(self, *exc):
        signal.alarm(0)


def tenant_paths(directory, n):
    """the tenant files, written where they are missing"""
    from synth_model import synth_model_blob
    os.makedirs(directory, exist_ok=True)
    paths = []
    for k in range(n):
        p = os.path.join(directory, "tenant40_%03d.kwsm" % k)
        if not os.path.exists(p):
            with open(p, "wb") as f:
                f.write(synth_model_blob(seed=8800 + k, ncep=40, num_filters=40, low=300, high=0, n_labels=LABELS[k % 3], logit_std=1.5))
        paths.append(p)
    return paths


def timed(torch, fn, steps, warmup):
    """seconds per step between two device events on the stream the calls are enqueued on"""
    for _ in range(warmup):
        fn()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(steps):
        fn()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1) * 1e-3 / steps


def measure(a):
    import torch
    assert torch.cuda.is_available(), "needs a GPU"
    from __graft_entry__ import load_package
    wanted = a.workloads.split(",")
    assert wanted and set(wanted) <= {"batch16", "live256", "batch256", "handles", "items"}, a.workloads
    dev = "items" in wanted
    assert not dev or wanted == ["items"], "the items workload runs alone, on the development library"
    pkg = load_package(dev=dev)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    fout = open(a.out, "a")
    missed = []

    def emit(**d):
        line = json.dumps(d)
        print(line, flush=True)
        fout.write(line + "\n")
        fout.flush()

    def run(workload, variants, check, **facts):
        """variants: name -> callable; alternating, a.repeats times"""
        with StepLimit(workload, a.limit):
            for fn in variants.values():
                fn()
            assert check(), "%s: the pool's rows differ from the other variant's" % workload
            times = {v: [] for v in variants}
            for _ in range(a.repeats):
                for v, fn in variants.items():
                    times[v].append(timed(torch, fn, a.steps, a.warmup))
        for v, ts in times.items():
            emit(workload=workload, variant=v, steps=a.steps, warmup=a.warmup, seconds_per_step=ts, median_ms=statistics.median(ts) * 1e3,
                 spread_ms=(max(ts) - min(ts)) * 1e3, same_bits=True, **facts)
        return {v: statistics.median(ts) for v, ts in times.items()}, {v: max(ts) - min(ts) for v, ts in times.items()}

    def bits(t):
        return t.view(torch.int32)

    # ---- the tenants: kws_create time and device bytes per handle
    paths = tenant_paths(a.tenants, TENANTS)
    n_models = TENANTS if set(wanted) & {"live256", "batch256", "handles", "items"} else BANK
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    t0 = time.perf_counter()
    models = [pkg.Model(p) for p in paths[:n_models]]
    torch.cuda.synchronize()
    dt, used = time.perf_counter() - t0, free0 - torch.cuda.mem_get_info()[0]
    assert all(m.nn_kernel == "kws_nn_mfma_kernel" for m in models)
    if "handles" in wanted:
        emit(workload="handles", variant="kws_create", handles=n_models, seconds_per_handle=dt / n_models, device_bytes_per_handle=used / n_models,
             file_bytes=os.path.getsize(paths[0]))
    clip, stride = models[0].clip_samples, max(LABELS)

    def batch_inputs():
        B = a.clips - a.clips % TENANTS
        pcm = torch.empty((B, clip), dtype=torch.int16, device="cuda")
        pkg.synth_clips_device(23, 0, B, clip, pcm.data_ptr())
        return B, pcm

    def members(kind, B, K):
        i = np.arange(B)
        if kind == "even":
            return (i % K).astype(np.uint32)
        m = (1 + (i // 2) % (K - 1)).astype(np.uint32)          # half: tenant 0 holds every second clip
        m[::2] = 0
        return m

    def pool_batch(pool, pcm, B, member):
        s = torch.zeros((B, stride), dtype=torch.float32, device="cuda")
        return s, (lambda: pool.run_classifier_device(pcm.data_ptr(), B, member, s.data_ptr()))

    def live_setup(pool, S):
        """a pool session in steady state: one window per stream and push; returns (push, scores, counts)"""
        per, n_push = S // TENANTS, 16
        pcm = torch.empty((S * n_push * SLICE // 16000 + 1, 16000), dtype=torch.int16, device="cuda")
        pkg.synth_clips_device(29, 0, pcm.shape[0], 16000, pcm.data_ptr())
        lv = pool.live_streams(S, SLICE)
        lv.assign(np.arange(S), (np.arange(S) // per).astype(np.uint32))          # streams [k per, (k + 1) per) -> tenant k
        sc = torch.zeros((S, stride), dtype=torch.float32, device="cuda")
        streams, lens = np.arange(S), np.full(S, SLICE)
        state = {"step": 0, "count": 0}

        def offs(step):
            return (np.arange(S) * n_push + step % n_push) * SLICE

        def push():
            state["count"] = int(lv.push_device(pcm.data_ptr(), streams, offs(state["step"]), lens, sc.data_ptr()).sum())
            state["step"] += 1
        return lv, pcm, sc, push, state, offs

    if "batch16" in wanted:
        gms = models[:BANK]
        pool, bank = pkg.Pool(gms), pkg.Bank(gms)
        B, pcm = batch_inputs()
        member = members("even", B, BANK)
        routes = (np.uint32(1) << member).astype(np.uint32)
        sp, f_pool = pool_batch(pool, pcm, B, member)
        sb = [torch.zeros((B, m.n_labels), dtype=torch.float32, device="cuda") for m in gms]

        def f_bank():
            bank.run_classifier_routed_device(pcm.data_ptr(), B, routes, [t.data_ptr() for t in sb])

        def check():
            torch.cuda.synchronize()
            return all(torch.equal(bits(sp)[k::BANK, :m.n_labels], bits(sb[k])[k::BANK]) and bool(sb[k][k::BANK].any()) for k, m in enumerate(gms))
        med, spread = run("batch16", {"pool": f_pool, "bank": f_bank}, check, clips=B, tenants=BANK, item_rows=pkg.lib().kws_pool_item_rows())
        if med["pool"] > med["bank"] + spread["bank"]:
            missed.append("bar 1: pool %.3f ms > routed bank %.3f ms + its spread %.3f ms" % (med["pool"] * 1e3, med["bank"] * 1e3, spread["bank"] * 1e3))
        torch.cuda.synchronize()
        pool.close()
        bank.close()
        del pcm, sp, sb

    if "batch256" in wanted:
        pool = pkg.Pool(models)
        B, pcm = batch_inputs()
        own = torch.zeros((B, models[0].n_labels), dtype=torch.float32, device="cuda")
        models[0].run_classifier_batch_device(pcm.data_ptr(), B, own.data_ptr(), None)
        for kind in ("even", "half"):
            member = members(kind, B, TENANTS)
            sp, f_pool = pool_batch(pool, pcm, B, member)

            def check(member=member, sp=sp):
                torch.cuda.synchronize()
                at = torch.from_numpy(np.nonzero(member == 0)[0]).cuda()           # tenant 0's rows against its own call
                return torch.equal(bits(sp)[at, :own.shape[1]], bits(own)[at])
            run("batch256_" + kind, {"pool": f_pool}, check, clips=B, tenants=TENANTS, rows_of_tenant_0=int((member == 0).sum()),
                item_rows=pkg.lib().kws_pool_item_rows())
            del sp
        torch.cuda.synchronize()
        pool.close()
        del pcm, own

    if "live256" in wanted:
        S = a.streams - a.streams % TENANTS
        per_bank = S // BANK
        pool = pkg.Pool(models)
        lv, pcm, sc, push_pool, state, offs = live_setup(pool, S)
        banks = [pkg.Bank(models[b * BANK:(b + 1) * BANK]) for b in range(BANK)]
        sessions = [bk.live_streams(per_bank, SLICE) for bk in banks]
        per = S // TENANTS
        for ses in sessions:                                                       # stream j of a bank -> its member j / per
            ses.route(np.arange(per_bank), (np.uint32(1) << (np.arange(per_bank) // per).astype(np.uint32)).astype(np.uint32))
        sb = [[torch.zeros((per_bank, m.n_labels), dtype=torch.float32, device="cuda") for m in bk.members] for bk in banks]
        bstate = {"step": 0, "count": 0}
        local, lens = np.arange(per_bank), np.full(per_bank, SLICE)

        def push_banks():
            o = offs(bstate["step"])
            bstate["count"] = sum(int(ses.push_device(pcm.data_ptr(), local, o[b * per_bank:(b + 1) * per_bank], lens, [t.data_ptr() for t in sb[b]]).sum())
                                  for b, ses in enumerate(sessions))
            bstate["step"] += 1

        def check():
            torch.cuda.synchronize()
            if state["step"] != bstate["step"] or state["count"] != S or bstate["count"] != S:
                return False
            for k, m in enumerate(models):
                b, j = divmod(k, BANK)
                if not torch.equal(bits(sc)[k * per:(k + 1) * per, :m.n_labels], bits(sb[b][j])[j * per:(j + 1) * per]):
                    return False
            return True
        for _ in range(16000 // SLICE + 3):                                        # up to steady state: a window per stream and push
            push_pool()
            push_banks()
        med, spread = run("live256", {"pool": push_pool, "banks": push_banks}, check, streams=S, tenants=TENANTS, slice_samples=SLICE,
                          item_rows=pkg.lib().kws_pool_item_rows())
        if med["pool"] + spread["pool"] >= med["banks"]:
            missed.append("bar 2: pool push %.3f ms + its spread %.3f ms >= sixteen routed-bank pushes %.3f ms" % (med["pool"] * 1e3, spread["pool"] * 1e3, med["banks"] * 1e3))
        torch.cuda.synchronize()
        lv.close()
        for ses in sessions:
            ses.close()
        for bk in banks:
            bk.close()
        pool.close()
        del pcm

    if "items" in wanted:
        pool16, pool = pkg.Pool(models[:BANK]), pkg.Pool(models)
        B, pcm = batch_inputs()
        S = a.streams - a.streams % TENANTS
        lv, lpcm, sc, push_pool, state, _ = live_setup(pool, S)
        for _ in range(16000 // SLICE + 3):
            push_pool()
        shapes = {}
        for name, pl, kind, K in (("batch16", pool16, "even", BANK), ("batch256_even", pool, "even", TENANTS), ("batch256_half", pool, "half", TENANTS)):
            shapes[name] = pool_batch(pl, pcm, B, members(kind, B, K))
        shapes["small_one"] = pool_batch(pool16, pcm, a.small, np.zeros(a.small, np.uint32))     # few clips, all of one tenant: the balance side of the trade
        shapes["live256"] = (sc, push_pool)
        first = {}
        with StepLimit("items", a.limit):
            times = {}
            for _ in range(a.repeats):
                for r in a.item_rows.split(","):
                    os.environ["KWS_DEV_POOL_ITEM_ROWS"] = r
                    assert pkg.lib().kws_pool_item_rows() == int(r)
                    for name, (out, fn) in shapes.items():
                        fn()
                        torch.cuda.synchronize()
                        if name != "live256":                                      # (a live push moves on: its rows differ from push to push)
                            assert torch.equal(bits(first.setdefault(name, out.clone())), bits(out)), "item size %s changes the bits of %s" % (r, name)
                        times.setdefault((name, int(r)), []).append(timed(torch, fn, a.steps, a.warmup))
        os.environ.pop("KWS_DEV_POOL_ITEM_ROWS", None)
        for (name, r), ts in times.items():
            emit(workload="items", variant=name, item_rows=r, steps=a.steps, warmup=a.warmup, seconds_per_step=ts, median_ms=statistics.median(ts) * 1e3,
                 spread_ms=(max(ts) - min(ts)) * 1e3, clips=a.small if name == "small_one" else B, streams=S, same_bits=True)
        torch.cuda.synchronize()
        lv.close()
        pool16.close()
        pool.close()
    for m in models:
        m.close()
    fout.close()
    if missed:
        print("a bar is missed: " + "; ".join(missed), file=sys.stderr)
        sys.exit(1)


def write_md(a):
    rows = [json.loads(ln) for ln in open(a.out) if ln.strip()]
    cells = {}
    for d in rows:
        # (a later line of the same cell replaces an earlier one; only the items workload has a cell per item size)
        cells.setdefault(d["workload"], {})[(d["variant"], d["item_rows"] if d["workload"] == "items" else None)] = d
    timed_rows = [d for d in rows if "steps" in d]
    first = timed_rows[0]
    out = ["# Pools: hundreds of int8 tenants behind one DSP block, one member per row", "",
           "One MI355X, KWS_MODE_EXACT kernels in every variant (pool and bank calls always run them), every variant in one process and library.  Tenants: "
           "synthetic int8 graphs of the stock two-block shape at 49 x 40 features, one seed each, 3 / 4 / 6 labels in turn.  Per variant: %d warm-up steps, "
           "then %d timed steps between two device events, the variants of a workload alternating, %d repeats; all repeats are listed, with their median and "
           "spread (max - min).  Before timing, the pool's rows were compared with the other variant's rows of the same (row, member) pairs: same bits.  Times "
           "are per step of the whole call on the device (enqueue to last kernel), not kernel times.  Written by tools/gpu_pool_rate.py."
           % (first["warmup"], first["steps"], len(first["seconds_per_step"])), ""]
    what = {("batch16", "pool"): "one pool call, clip i -> tenant i mod 16", ("batch16", "bank"): "one routed bank call, one-hot round-robin routes",
            ("live256", "pool"): "one push of one pool session", ("live256", "banks"): "sixteen routed-bank pushes, 16 banks of 16 members, back to back",
            ("batch256_even", "pool"): "one pool call, clip i -> tenant i mod 256", ("batch256_half", "pool"): "one pool call, tenant 0 holds every second clip"}

    def table(w):
        t = ["| variant | median ms | spread ms | every repeat, ms |", "|---|---|---|---|"]
        for (v, _), d in cells[w].items():
            t.append("| %s | %.3f | %.3f | %s |" % (what[(w, v)], d["median_ms"], d["spread_ms"], " ".join("%.3f" % (x * 1e3) for x in d["seconds_per_step"])))
        return t + [""]
    if "batch16" in cells:
        p, b = cells["batch16"][("pool", None)], cells["batch16"][("bank", None)]
        out += ["## Bar 1: %d resident clips, 16 tenants, round robin (work items of %d rows)" % (p["clips"], p["item_rows"]), ""] + table("batch16")
        out += ["The bar: the pool call's median (%.3f ms) must not exceed the routed bank call's (%.3f ms) by more than the spread between the latter's repeats "
                "(%.3f ms): %s." % (p["median_ms"], b["median_ms"], b["spread_ms"], "met" if p["median_ms"] <= b["median_ms"] + b["spread_ms"] else "MISSED"), ""]
    if "live256" in cells:
        p, b = cells["live256"][("pool", None)], cells["live256"][("banks", None)]
        out += ["## Bar 2: %d live streams of 256 tenants, one 250 ms slice per push" % p["streams"], ""] + table("live256")
        out += ["The bar: the pool push's median plus the spread between its repeats (%.3f + %.3f ms) must stay below the sixteen routed-bank pushes' median "
                "(%.3f ms): %s." % (p["median_ms"], p["spread_ms"], b["median_ms"], "met" if p["median_ms"] + p["spread_ms"] < b["median_ms"] else "MISSED"), ""]
    for w, title in (("batch256_even", "even"), ("batch256_half", "one tenant holds half")):
        if w in cells:
            d = cells[w][("pool", None)]
            out += ["## Recorded: %d resident clips, 256 tenants, %s (tenant 0: %d rows)" % (d["clips"], title, d["rows_of_tenant_0"]), ""] + table(w)
    if "handles" in cells:
        d = cells["handles"][("kws_create", None)]
        out += ["## Recorded: what a tenant handle costs", "",
                "%d handles made one after the other from files of %d bytes: %.2f ms of kws_create and %.0f bytes of device memory per handle (the device's free "
                "memory before and after; the allocator's granules included)." % (d["handles"], d["file_bytes"], d["seconds_per_handle"] * 1e3, d["device_bytes_per_handle"]), ""]
    if "items" in cells:
        names = ["batch16", "batch256_even", "batch256_half", "small_one", "live256"]
        sizes = sorted({r for (_, r) in cells["items"]})
        out += ["## Recorded: rows per work item (KWS_POOL_ITEM_ROWS)", "",
                "The development library, its KWS_DEV_POOL_ITEM_ROWS switch set between calls in one process; median ms (spread) of the pool call on each shape; "
                "the scores of every batch shape are the same bits at every size.  small_one: %d clips that all name one tenant of 16 -- the case in which large "
                "items leave workgroups idle." % cells["items"][("small_one", sizes[0])]["clips"], "",
                "| rows per item | " + " | ".join(names) + " |", "|---|" + "---|" * len(names)]
        for r in sizes:
            out.append("| %d | " % r + " | ".join("%.3f (%.3f)" % (cells["items"][(n, r)]["median_ms"], cells["items"][(n, r)]["spread_ms"]) for n in names) + " |")
        out += ["", "What the table decides (csrc/kws_pool.h): large items spare the staging of a member's tables (12 KB per workgroup) and win a little where the "
                "batch is large; small items keep every CU busy where one tenant holds most of a small batch; the live push, whose lists are a few rows long, does "
                "not feel the setting.  KWS_POOL_ITEM_ROWS is the size that stays within a few percent of the best on both sides.", ""]
    os.makedirs(os.path.dirname(os.path.abspath(a.md)), exist_ok=True)
    open(a.md, "w").write("\n".join(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="batch16,live256,batch256,handles")
    ap.add_argument("--clips", type=int, default=65536)
    ap.add_argument("--streams", type=int, default=1024)
    ap.add_argument("--item-rows", default="4,8,16,32,64")
    ap.add_argument("--small", type=int, default=4096, help="clips of the items workload's small_one shape")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--limit", type=int, default=150, help="seconds each workload may take")
    ap.add_argument("--tenants", default=os.path.join(ROOT, "build", "pool_tenants"), help="directory of the tenant files (written where missing)")
    ap.add_argument("--make-tenants", action="store_true", help="write the tenant files and stop (host only)")
    ap.add_argument("--out", default=os.path.join(ROOT, "build", "pool_rate.jsonl"))
    ap.add_argument("--md", default=None, help="write the tables from --out; runs nothing")
    a = ap.parse_args()
    if a.make_tenants:
        tenant_paths(a.tenants, TENANTS)
    elif a.md:
        write_md(a)
    else:
        measure(a)


if __name__ == "__main__":
    main()
