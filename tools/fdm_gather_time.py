#!/usr/bin/env python3
"""Wall time of `hipla.fdm.gather_factors` (the factors read off the resident matrix) next to the
host's `inverse_factors` (extraction and proof) on the same velocity operator: one process, five interleaved rounds,
medians, and the check that the gathered factors equal the host's.  Results: profiles/fdm_gather.md.

    python tools/fdm_gather_time.py [--sizes 3:32 3:64 3:96] [--rounds 5]

Prints one line per size and one JSON line at the end."""

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "navier-stokes-solver_amd"))

import numpy as np

import hipla
from hipla import fdm
from staggered_grid import mac_stokes


def measure(dim, n, rounds):
    s = mac_stokes(dim, n, 0.01)
    A = hipla.SparseMatrix.from_scipy(s.A)
    components = [np.asarray(g, dtype=np.int64) for g in s.component_ids]
    bases, pitch = fdm._affine_layout(components, s.n_u)
    shapes = [g.shape for g in components]
    fdm.gather_factors(A, bases, pitch, shapes)              # (the first launch loads the kernel)
    gather, host = [], []
    for _ in range(rounds):
        t0 = time.perf_counter()
        T = fdm.gather_factors(A, bases, pitch, shapes)
        t1 = time.perf_counter()
        made, why = fdm.inverse_factors(s.A, s.component_ids)
        t2 = time.perf_counter()
        gather.append(t1 - t0)
        host.append(t2 - t1)
    assert why is None and all(np.array_equal(a, b) for ts, f in zip(T, made.factors) for a, b in zip(ts, f.T))
    return {"rows": int(s.n_u), "gather_s": float(np.median(gather)), "host_inverse_factors_s": float(np.median(host))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", nargs="+", default=["3:32", "3:64", "3:96"], help="dim:n")
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    out = {}
    for size in args.sizes:
        dim, n = (int(x) for x in size.split(":"))
        out["%dd_n%d" % (dim, n)] = got = measure(dim, n, args.rounds)
        print(dim, n, got, flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
