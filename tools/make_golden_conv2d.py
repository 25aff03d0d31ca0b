#!/usr/bin/env python3
"""Writes tests/golden/conv2d_graphs.npz: for every graph of tests/conv2d_testlib.py CONV2D_SPECS, what the compiled REFERENCE (oracle/_ref, its own
TFLite-Micro op registrations through Reference.graph_run) computes: the int8 graph's output rows on conv2d_features(), the float twin's score rows on
conv2d_twin_features(), and one digest per conv block output, hidden tensor and logits tensor of both (float tensors with every NaN as the one quiet
pattern: NaN is compared by position).  The oracle must reproduce it (tests/test_conv2d_graphs_host.py): that is what pins the oracle on a machine
without the reference.  The maker refuses a graph that is vacuous (saturated block outputs, too few distinct rows, one class winning everything).

usage: make_golden_conv2d.py          (needs oracle/_ref: __graft_entry__.build() with the reference sources present)
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import conv2d_testlib as T  # noqa: E402
import dense_testlib as D  # noqa: E402
from kws_testlib import Oracle, Reference, have_reference  # noqa: E402


def main():
    if not have_reference():
        sys.exit("oracle/_ref is not built")
    ref, oracle = Reference(), Oracle()
    out = {}
    for name in T.CONV2D_SPECS:
        blob, twin = T.conv2d_blob(name), T.conv2d_twin(name)
        m = D.oracle_model(oracle, blob)
        ids = T.tensor_ids(blob)
        q_rows, f_rows, q_t, f_t = [], [], {i: [] for i in ids}, {i: [] for i in ids}
        for row in T.conv2d_features(name):
            o, t = ref.graph_run(blob, m.quantize_input(row))
            q_rows.append(o.copy())
            for i in ids:
                q_t[i].append(t[i].copy())
        for row in T.conv2d_twin_features(name):
            o, t = ref.graph_run(twin, row)
            f_rows.append(o.copy())
            for i in ids:
                f_t[i].append(t[i].copy())
        q_rows, f_rows = np.stack(q_rows), np.stack(f_rows)
        T.check_not_vacuous(name, blob, {i: np.stack(q_t[i]) for i in ids}, q_rows, f_rows)
        out[name + "/scores"] = q_rows
        out[name + "/fscores"] = f_rows
        out[name + "/digests"] = np.array([D.digest(np.stack(q_t[i])) for i in ids] + [D.digest(T.canonical_nan(np.stack(f_t[i]))) for i in ids], np.uint64)
        print(name, q_rows.shape, f_rows.shape, len(ids), "tensors")
    np.savez_compressed(T.GOLDEN_CONV2D, **out)
    print(T.GOLDEN_CONV2D, os.path.getsize(T.GOLDEN_CONV2D), "bytes")


if __name__ == "__main__":
    main()
