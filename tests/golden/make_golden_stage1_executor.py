#!/usr/bin/env python3
"""Generates tests/golden/stage1_executor_step.npz: one step of engine_stage1.Stage1Engine on the uncontracted case of
tests/stage1_executor_case.py, recorded on a gfx950 device from the commit BEFORE the executor's gather learnt to contract (the parent of
the commit that added n2m_gather_contract_x01).  tests/test_stage1_contract_gpu.py holds the current executor, `contract` off, to these
bits.  The step is recorded three times from the same seeded state; an array that differs between the recordings (float atomics: the
vertex offsets) is listed in `unstable` and kept from all three (`offsets`, `offsets_b`, `offsets_c`), so that the test can hold the
current code to the distance between them.

    python tests/golden/make_golden_stage1_executor.py [--out PATH]
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import stage1_executor_case as EC        # noqa: E402


def main():
    path = os.path.join(HERE, "stage1_executor_step.npz")
    if "--out" in sys.argv:
        path = sys.argv[sys.argv.index("--out") + 1]
    a, b, c = EC.record(), EC.record(), EC.record()
    unstable = sorted(k for k in a if not (EC.same_bits(a[k], b[k]) and EC.same_bits(a[k], c[k])))
    for k in a:
        print(f"{k:14s} {str(np.asarray(a[k]).shape):12s} {'DIFFERS between recordings' if k in unstable else 'same bits in three recordings'}")
    for k in unstable:
        a[k + "_b"], a[k + "_c"] = b[k], c[k]
    a["unstable"] = np.array(unstable, dtype="U32")
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    np.savez_compressed(path, **a)
    print(f"loss {a['loss']:.6f}, covered {a['covered']}, table entries moved {a['table_moved']}, {os.path.getsize(path) / 1024:.0f} KiB -> {path}")


if __name__ == "__main__":
    main()
