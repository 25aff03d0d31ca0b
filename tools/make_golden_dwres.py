#!/usr/bin/env python3
"""Writes tests/golden/dwres_graphs.npz: for every graph of tests/dwres_testlib.py DW_SPECS, what the compiled REFERENCE (oracle/_ref, its own TFLite-Micro
op registrations -- Register_DEPTHWISE_CONV_2D among them -- through Reference.graph_run) computes: the int8 graph's output rows on res_features(), the
float twin's output rows on res_twin_features() as bit patterns, and one digest per step output, hidden tensor and logits tensor of both (float tensors
with every NaN as the one quiet pattern: NaN is compared by position).  The oracle must reproduce the file (tests/test_dwres_graphs_host.py): that is what
pins the oracle on a machine without the reference.  The maker refuses a graph that is vacuous (dwres_testlib.check_not_vacuous).

usage: make_golden_dwres.py          (needs oracle/_ref: __graft_entry__.build() with the reference sources present)
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import dense_testlib as D  # noqa: E402
import dwres_testlib as T  # noqa: E402
from kws_testlib import Oracle, Reference, have_reference  # noqa: E402


def main():
    if not have_reference():
        sys.exit("oracle/_ref is not built")
    ref, oracle = Reference(), Oracle()
    out = {}
    for name in T.DW_SPECS:
        blob, twin = T.dw_blob(name), T.dw_twin(name)
        m = D.oracle_model(oracle, blob)
        ids, watched = T.tensor_ids(blob), T.watched_ids(blob)
        q_rows, f_rows, q_t, f_t = [], [], {i: [] for i in watched}, {i: [] for i in ids}
        for row in T.res_features():
            o, t = ref.graph_run(blob, m.quantize_input(row))
            q_rows.append(o.copy())
            for i in watched:
                q_t[i].append(t[i].copy())
        for row in T.res_twin_features():
            o, t = ref.graph_run(twin, row)
            f_rows.append(o.copy())
            for i in ids:
                f_t[i].append(t[i].copy())
        q_rows, f_rows = np.stack(q_rows), np.stack(f_rows)
        T.check_not_vacuous(name, blob, {i: np.stack(q_t[i]) for i in watched}, q_rows, f_rows)
        out[name + "/scores"] = q_rows
        out[name + "/fscores"] = np.ascontiguousarray(f_rows, np.float32).view(np.uint32)
        out[name + "/digests"] = np.array([D.digest(np.stack(q_t[i])) for i in ids] + [D.digest(T.canonical_nan(np.stack(f_t[i]))) for i in ids], np.uint64)
        print(name, q_rows.shape, f_rows.shape, len(ids), "tensors")
    np.savez_compressed(T.GOLDEN_DWRES, **out)
    print(T.GOLDEN_DWRES, os.path.getsize(T.GOLDEN_DWRES), "bytes")


if __name__ == "__main__":
    main()
