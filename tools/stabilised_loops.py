#!/usr/bin/env python3
"""Time per iteration of the textbook BPCG and MINRES on a stabilised system [[A, B^T], [B, C]] with
C = pressure_stabilisation(eps) (profiles/stabilised_loops.md):

  protocol   the entry point statement by statement (hipla.fused.ENABLED = False) with C -- what ran before the fused
             loops took a C: time(n2 iterations) - time(n1 iterations) over n2 - n1, each ending in a download
  fused+C    the device loop with C:    the time of the loop's run() over its iterations (tolerance 0)
  fused      the device loop, C = None: likewise, same A and B

One window of each per call, in that order; the caller alternates calls (and libraries: NSS_LIB_PATH names another
build, whose loops know no C -- then only `fused` is measured) and takes medians.  One JSON line per figure.

    python tools/stabilised_loops.py --dim 2 --n 183 [--iters 2000] [--out FILE]
"""

import argparse
import contextlib
import io
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "navier-stokes-solver_amd")]

import numpy as np                                   # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dim", type=int, required=True)
    ap.add_argument("--n", type=int, required=True)
    ap.add_argument("--eps", type=float, default=1.0)
    ap.add_argument("--iters", type=int, default=2000)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import hipla
    from hipla import fused
    from bramble_pasciak_cg import bramble_pasciak_cg
    from minres import MinRes
    from staggered_grid import mac_stokes

    hipla.set_engine(None)
    eng = hipla.get_engine()
    other_build = bool(os.environ.get("NSS_LIB_PATH"))
    s = mac_stokes(args.dim, args.n, 0.01)
    Cs = s.pressure_stabilisation(args.eps)
    f = s.rhs(0)[0]
    g = np.random.default_rng(1).standard_normal(s.n_p)
    g -= g.mean()
    A, B = hipla.SparseMatrix.from_scipy(s.A), hipla.SparseMatrix.from_scipy(s.B)
    Cm = hipla.SparseMatrix.from_scipy(Cs)
    preA, preS = hipla.DiagonalMatrix(1.0 / s.A.diagonal()), hipla.DiagonalMatrix(1.0 / s.mass)
    fv, gv = hipla.Vector.from_numpy(f), hipla.Vector.from_numpy(g)

    spent = {}
    for key, cls in (("bpcg1", fused.Bpcg1Loop), ("minres", fused.MinresLoop)):
        def timed(self, *a, _key=key, _orig=cls.run, **kw):
            t0 = time.perf_counter()
            out = _orig(self, *a, **kw)                # (ends in a poll and the download of the history)
            spent[_key] = time.perf_counter() - t0
            return out
        cls.run = timed

    def call(solver, c, steps):
        t0 = time.perf_counter()
        with contextlib.redirect_stdout(io.StringIO()):
            if solver == "bpcg1":
                sol, _ = bramble_pasciak_cg(A, B, c, preA, preS, fv, gv, tolerance=0.0, max_steps=steps, print_rates=False)
            else:
                sol, _ = MinRes(mat=hipla.BlockMatrix([[A, B.T], [B, c]]), pre=hipla.BlockMatrix([[preA, None], [None, preS]]),
                                rhs=hipla.BlockVector([fv, gv]), maxsteps=steps, tol=0.0, printrates=False)
        sol.numpy()
        return time.perf_counter() - t0

    rows = []
    for solver in ("bpcg1", "minres"):
        variants = [("fused", None)] if other_build else [("protocol", Cm), ("fused+C", Cm), ("fused", None)]
        for variant, c in variants:
            spent.clear()
            fused.ENABLED = variant != "protocol"
            call(solver, c, 40)                      # warm-up of every kernel the window uses
            if variant == "protocol":
                n1, n2 = 50, 50 + max(200, args.iters // 4)
                us = (call(solver, c, n2) - call(solver, c, n1)) / (n2 - n1) * 1e6
                assert not spent, "the fused loop ran in the protocol window"
            else:
                call(solver, c, args.iters)
                assert solver in spent, (fused.Bpcg1Loop.last_declined, fused.MinresLoop.last_declined)
                us = spent[solver] / args.iters * 1e6
            fused.ENABLED = True
            rows.append(dict(solver=solver, variant=variant, dim=args.dim, n=args.n, dof=s.ndof, nnz_c=int(Cs.nnz),
                             us_per_iteration=round(us, 3), library="other" if other_build else "own", engine=eng.name))
    text = "\n".join(json.dumps(r) for r in rows)
    print(text)
    if args.out:
        with open(args.out, "a") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
