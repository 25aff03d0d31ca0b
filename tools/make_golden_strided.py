#!/usr/bin/env python3
"""Writes tests/golden/strided_graphs.npz: for every graph of tests/strided_testlib.py STRIDED_SPECS, what the compiled REFERENCE (oracle/_ref, its own
TFLite-Micro op registrations through Reference.graph_run) computes on strided_features(): the int8 graph's output rows, the float twin's score rows
and one digest per conv block output, hidden tensor and logits tensor of both.  The oracle must reproduce it (tests/test_strided_graphs_host.py): that
is what pins the oracle on a machine without the reference.  The maker refuses a graph that is vacuous (saturated block outputs, too few distinct rows).

usage: make_golden_strided.py          (needs oracle/_ref: __graft_entry__.build() with the reference sources present)
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import dense_testlib as D  # noqa: E402
import strided_testlib as S  # noqa: E402
from kws_testlib import Oracle, Reference, have_reference  # noqa: E402


def main():
    if not have_reference():
        sys.exit("oracle/_ref is not built")
    ref, oracle = Reference(), Oracle()
    out = {}
    for name in S.STRIDED_SPECS:
        blob, twin, f = S.strided_blob(name), S.strided_twin(name), S.strided_features(name)
        _, _, hidden, last, _, _ = D.graph_layout(blob)
        m = D.oracle_model(oracle, blob)
        ids = D.block_outputs(blob) + hidden + [last]
        q_rows, f_rows, q_t, f_t = [], [], {i: [] for i in ids}, {i: [] for i in ids}
        for row in f:
            o, t = ref.graph_run(blob, m.quantize_input(row))
            q_rows.append(o.copy())
            for i in ids:
                q_t[i].append(t[i].copy())
            o, t = ref.graph_run(twin, row)
            f_rows.append(o.copy())
            for i in ids:
                f_t[i].append(t[i].copy())
        q_rows, f_rows = np.stack(q_rows), np.stack(f_rows)
        S.check_not_vacuous(name, blob, {i: np.stack(q_t[i]) for i in ids}, q_rows, f_rows)
        out[name + "/scores"] = q_rows
        out[name + "/fscores"] = f_rows
        out[name + "/digests"] = np.array([D.digest(np.stack(q_t[i])) for i in ids] + [D.digest(np.stack(f_t[i])) for i in ids], np.uint64)
        print(name, q_rows.shape, len(ids), "tensors")
    np.savez_compressed(S.GOLDEN_STRIDED, **out)
    print(S.GOLDEN_STRIDED, os.path.getsize(S.GOLDEN_STRIDED), "bytes")


if __name__ == "__main__":
    main()
