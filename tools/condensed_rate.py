"""Iteration rate of the statically condensed BPCG path (scope row N2; fused and statement by
statement) next to the fused uncondensed loop:  python tools/condensed_rate.py [grid] [--mypre]

--mypre: the reference's default preconditioner instead of point Jacobi -- MypreA(GS=True) with the auxiliary-space
term, over A (uncondensed) or over the Schur complement with blocks of coupling dofs (condensed); the set-up column
then holds the scale factor's Lanczos (device-resident on the fused rows, protocol recurrence on the last)."""
import contextlib
import io
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "navier-stokes-solver_amd"))

import numpy as np

import hipla
from discretizations import CondensedForm
from solvers.bramblepasciak_new import BramblePasciakCG
from staggered_grid import mac_stokes


class Form:
    def __init__(self, mat):
        self.mat, self.condense = mat, False


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    mypre = "--mypre" in sys.argv
    grid = int(args[0]) if args else 96
    s = mac_stokes(3, grid, 0.01)
    if mypre:
        from templates.NavierStokesSIMPLE_iterative import MypreA, auxiliary_space_preconditioner, coupling_blocks
        _, _, aux = auxiliary_space_preconditioner(s)
    f, g = s.rhs(0)
    eng = hipla.get_engine()
    B = hipla.SparseMatrix.from_scipy(s.B)
    preS = hipla.DiagonalMatrix(1.0 / s.mass)
    rows = []
    from hipla import fused
    for label in ("uncondensed, fused loop", "condensed, fused loop (explicit product + harmonic_extension step)",
                  "condensed, protocol statements"):
        fused.ENABLED = not label.endswith("statements")
        if label.startswith("uncondensed"):
            A = hipla.SparseMatrix.from_scipy(s.A)
            blfA = Form(A)
            preA = MypreA(None, blfA, s.facet_blocks(), GS=True, aux=aux) if mypre else hipla.JacobiPreconditioner(A)
        else:
            blfA = CondensedForm(s)
            preA = (MypreA(None, blfA, coupling_blocks(s.facet_blocks(), blfA.interior), GS=True, aux=aux) if mypre
                    else blfA.jacobi())
        for _ in range(2):                                           # the second, warm solve is reported
            sol = hipla.BlockVector([hipla.Vector(s.n_u), hipla.Vector(s.n_p)])
            out = io.StringIO()
            eng.synchronize()
            t0 = time.perf_counter()
            with contextlib.redirect_stdout(out):
                it, seconds = BramblePasciakCG(blfA, Form(B), None, hipla.Vector.from_numpy(f),
                                               hipla.Vector.from_numpy(g), preA, preS, sol, tol=1e-6, maxsteps=400)
            eng.synchronize()
            setup = time.perf_counter() - t0 - seconds               # session: Lanczos of k, right-hand side, defect
        x = sol.numpy()
        res = np.linalg.norm(np.concatenate([f, g]) - s.saddle_matrix() @ x) / np.linalg.norm(np.concatenate([f, g]))
        rows.append((label, it, seconds, 1e3 * seconds / max(it, 1), setup, res))
    print("3-D MAC Stokes n=%d, %d DoF, BPCG v2, %s, 400 iterations max"
          % (grid, s.ndof, "MypreA(GS=True) + auxiliary term" if mypre else "point Jacobi"))
    print("| path | iterations | loop s | ms / iteration | set-up s | true residual |\n|---|---|---|---|---|---|")
    for r in rows:
        print("| %s | %d | %.3f | %.3f | %.3f | %.1e |" % r)


if __name__ == "__main__":
    main()
