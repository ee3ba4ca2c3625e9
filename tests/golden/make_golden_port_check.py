#!/usr/bin/env python3
"""Emit tests/golden/port_check_golden.npz from the REFERENCE's own CPU library (oracle/_ref, build container only): the case of
tests/test_oracle.py::test_port_vs_live_reference_library -- make_problem(1500, 700, 9, seed=77), B = make_B(k, 9, seed=5) -- with its inputs and
what the reference's dgemm_compressed wrote for 'N' / 'T', uncentred / centred (cores = 8).  Fixtures are data only."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from _util import have_reference, make_B, make_problem, run_reference  # noqa: E402


def main():
    assert have_reference(), "build the reference first: make -C oracle ref"
    prob = make_problem(1500, 700, 9, seed=77)
    out = {"plink": prob["plink"], "plink_t": prob["plink_t"], "f": prob["f"], "dims": np.array([1500, 700, 9, 8], np.int64)}
    for trans in (0, 1):
        B = make_B(700 if trans else 1500, 9, seed=5)
        out[f"B{trans}"] = B
        for centered in (0, 1):
            out[f"C{trans}{centered}"], _ = run_reference(prob, trans, B, centered, cores=8)
    dst = os.path.join(HERE, "port_check_golden.npz")
    np.savez_compressed(dst, **out)
    print("wrote", dst, os.path.getsize(dst), "bytes")


if __name__ == "__main__":
    main()
